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
import random
import time

import pytest

import header_vectors
import path_harness as H

import make_header_vectors  # noqa: I100  (tools/, which path_harness has put on the path)

pytestmark = pytest.mark.gpu
LW = header_vectors.FLAG_LARGE_WINDOW


def _family(family):
    return [(e, c) for e, c in header_vectors.load() if e["family"] == family]


@pytest.mark.parametrize("family", ["P", "C", "B", "M"])
def test_every_vector_whole_short_truncated_and_damaged(pkg, family):
    """every stream of tests/golden/emitter_headers/ with exact, one-short, half and roomy output buffers (a random one too:
    path_harness.variants) and two truncated and two bit-flipped copies each; the one of 16 MiB of output exact and one short;
    without FLAG_LARGE_WINDOW and with it (the large-window streams: with it); batches of at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2019)
    by_flags = {0: ([], []), LW: ([], [])}
    for e, comp in _family(family):
        datas, caps = by_flags[header_vectors.flags_of(e)]
        if header_vectors.big(e):
            datas += [comp, comp]; caps += [e["size"], e["size"] - 1]
            continue
        d, c = H.variants(rnd, comp, e["size"], "tails")
        datas += d; caps += c
        if not e["large"]:
            by_flags[LW][0].extend(d); by_flags[LW][1].extend(c)
    n = 0
    for flags, (datas, caps) in by_flags.items():
        H.in_batches(pkg, datas, caps, None, flags, family)
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
        H.in_batches(pkg, datas, caps, None, flags, "%s%s cuts" % (family, slot))
    assert n >= 40
    print("wall time %.1f s, %d vectors, %d streams" % (time.time() - t0, n, sum(len(d) for d, _ in by_flags.values())))


def test_the_other_setting_of_the_large_window_flag(pkg):
    """every vector whole under FLAG_LARGE_WINDOW (a stream of a standard window decodes alike), and the large-window streams --
    the distance codes whose max_symbol lies below their alphabet among them -- without it (E_WINDOW_BITS)"""
    t0 = time.time()
    vectors = [(e, c) for e, c in header_vectors.load() if not header_vectors.big(e)]
    H.in_batches(pkg, [c for e, c in vectors], [header_vectors.cap_of(e) for e, c in vectors], None, LW, "with the flag")
    large = [(e, c) for e, c in vectors if e["large"]]
    assert len(large) >= 80
    results = H.check(pkg, [c for e, c in large], [header_vectors.cap_of(e) for e, c in large], None, 0, "without the flag")
    assert all((r.result, r.error_code) == (0, -13) for r in results)
    print("wall time %.1f s, %d + %d streams" % (time.time() - t0, len(vectors), len(large)))


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """header_vectors.leg_set (two batches, each led by a stream of more than 64 KiB, the size from which a launch forms gangs) in
    a fresh process per leg of path_harness.LEGS.  All legs return the oracle's status words and SHA-256s, and one another's.
    `engine_commands` says which path ran and is printed per leg; what the code guarantees is asserted: none without records, some
    for B's long form (a switch every 1 .. 40 symbols in each category, no context modelling) under the record loop, and gangs in
    the gang leg."""
    t0 = time.time()
    got = H.run_legs(header_vectors, show=lambda label, row: "/" not in label and row[H.COMMANDS] >= 40)
    eng = lambda name, label: got[name]["rows"][label][H.ENGINE]
    assert all(r[H.ENGINE] == 0 for r in got["norec"]["rows"].values())
    assert eng("records", "B-long") > 0, eng("records", "B-long")
    assert all(g >= 2 for g in got["gang8"]["gangs"]) and len(got["gang8"]["gangs"]) == 2, got["gang8"]["gangs"]
    print("wall time %.1f s, %d streams a leg" % (time.time() - t0, len(got["general"]["rows"])))


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
            results = H.check(pkg, datas, caps, None, flags | spill, "arena %d spill %d" % (arena, spill), batch)
            batch.close()
            if spill and flags == 0 and arena == 256:
                assert sum(r.spilled_metablocks for r in results) > 0
    print("wall time %.1f s" % (time.time() - t0))


def test_one_wave_blocks(pkg):
    """4 * CUs + 1 streams cycling over eight vectors: more than four blocks a CU, which are blocks of one wave and the small
    automatic arena whatever the streams are"""
    t0 = time.time()
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    eight = [by[n] for n in ("B-long", "B-lit-n256-ring", "C-imtf-every-tree-r9", "C-some-types-trivial", "P-cmd-depth-sixteens", "P-lit-one-16", "P-cmd-16chain-k5-e3",
                             "P-lit-V-seventeens-21")]
    _, n = H.blocks_a_cu(pkg, eight, cap_of=header_vectors.cap_of)
    print("wall time %.1f s, %d streams" % (time.time() - t0, n))


def _probe_streams(cus):
    """CUs + 1 streams with a mean of 8 KiB or more compressed: the vectors of 256 block types, B's long form and its
    every-length-code streams, and headers with faults behind a stored metablock of 8 KiB (make_header_vectors.behind_stored)"""
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    pool = [(c, header_vectors.cap_of(e)) for e, c in (by[n] for n in ("B-long", "B-lit-n256-ring", "B-lit-every-length-code", "B-lit-n255-direct",
                                                                          "B-cmd-every-length-code", "B-long", "B-dist-every-length-code", "B-lit-n256-direct"))]
    pool += [(c, len(raw) + 64) for _, c, raw in make_header_vectors.behind_stored()]
    n = cus + 1
    streams = [pool[i % len(pool)] for i in range(n)]
    assert sum(len(c) for c, _ in streams) >= 8192 * n, sum(len(c) for c, _ in streams) / n
    return streams


def _probe_batch(pkg):
    import torch
    streams = _probe_streams(torch.cuda.get_device_properties(0).multi_processor_count)
    results = H.check(pkg, [c for c, _ in streams], [cap for _, cap in streams], None, 0, "probe")
    return [len(streams), sum(1 for r in results if r.result == 1)]


def test_the_launch_that_asks_first(pkg):
    """a batch of CUs + 1 streams with a mean of 8 KiB or more compressed is one the launch asks the device about first: that
    launch decodes the distance context map and both tree groups in code of its own.  In a child with BROTLI_AMD_DEBUG_PROBE=1:
    stderr shows that it ran, and every result is the oracle's."""
    t0 = time.time()
    (n, good), stderr = H.in_a_child("test_gpu_headers", "_probe_batch", {"BROTLI_AMD_DEBUG_PROBE": "1"})
    assert "probe: %d streams" % n in stderr, stderr[-2000:]
    assert 0 < good < n
    print(stderr.strip().splitlines()[-1])
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
        out = H.streamed_like_the_model(pkg, comp, ic, oc, e["label"])
        assert out == header_vectors.expected(comp, e["size"], header_vectors.flags_of(e))[1] and hashlib.sha256(out).hexdigest()[:16] == e["sha"], e["label"]
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(streams)))


def test_four_vectors_in_a_stream_set(pkg):
    """one vector of each family with chunks (64, 37): four states stepped by a StreamSet and the same four stepped alone give the
    same calls and bytes, and the bytes are the oracle's"""
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    t0 = time.time()
    names = ["P-cmd-depth-sixteens", "C-imtf-every-tree-r9", "B-ones-all", "M-metadata-run-200x1"]
    jobs = [dict(data=by[n][1], ic=64, oc=37, lw=False) for n in names]
    want = [header_vectors.expected(by[n][1], by[n][0]["size"], 0)[1] for n in names]
    assert [hashlib.sha256(exp).hexdigest()[:16] for exp in want] == [by[n][0]["sha"] for n in names]
    H.stream_set_like_solo(pkg, jobs, names, want)
    print("wall time %.1f s" % (time.time() - t0))
