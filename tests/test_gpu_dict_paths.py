"""Custom (LZ77 prefix) dictionaries on every command path of the device and in every window regime (needs a real MI355X).

The kernels restate a dictionary's arithmetic in several places: the lean loop makes a copy out of the dictionary itself in two
parts split at position 0, the record loop takes a byte a lane from either side of it (from_cdict), the checked loop has
cdict_copy for every other shape, the path engine ends a pass at a distance into the dictionary and moves its word numbers by
the dictionary's size (pe_dict_word, classify), the gangs' form decides from the dictionary's size whether a reference beyond P
ends it, and the setup clamps what is in reach of a dictionary longer than the window.  The streams of tests/golden/emitter_dict/
(tools/make_dict_vectors.py, pinned on the CPU by test_emitter_dict_cpu.py) hold every shape by construction; here they go through
each path with their dictionaries.  Every comparison is path_harness.compare: result, error code, decoded size, every delivered
byte, and for successes consumed, num_commands, num_metablocks -- against brotli_oracle_decode_dict."""
import random
import time

import pytest

import dict_vectors
import path_harness as H
import stream_model as sm

import make_dict_vectors as M  # noqa: I100  (tools/, which path_harness has put on the path)

pytestmark = pytest.mark.gpu


def test_every_vector_whole_short_truncated_and_damaged(pkg):
    """every stream of tests/golden/emitter_dict/ with its dictionary: the valid ones with exact, short, half and roomy output buffers
    and two truncated and two bit-flipped copies each, the invalid ones as they are (roomy, and one byte short of what the oracle
    delivers); batches of at most 240 streams, a dictionary that several streams share as one object"""
    t0 = time.time()
    rnd = random.Random(2019)
    datas, caps, dicts = [], [], []
    for e, comp, d in dict_vectors.load():
        if e["valid"]:
            a, b = H.variants(rnd, comp, e["size"], "dict")
        else:
            a, b = [comp, comp], [e["size"] + 64, max(0, e["oracle"][2] - 1)]
        datas += a; caps += b; dicts += [d] * len(a)
    H.in_batches(pkg, datas, caps, dicts, what="vectors")
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """dict_vectors.leg_set (two batches, each led by F's long form of more than 64 KiB, the size from which a launch forms gangs) with
    its dictionaries in a fresh process per leg of path_harness.LEGS, the seven side by side: the path engine's one-block form,
    whatever the launch picks, gangs of eight, the scan engine, the command records, the checked loop alone, and no records at all.
    All legs return the same status words and SHA-256s, and those are the oracle's.  `engine_commands` says which path ran: on the
    carriers it is above 0 in the general, records, scan and gang8 legs; the share is printed, not judged -- nobody has measured
    what the engines take of a stream made for its dictionary (test_gpu_custom_dict.test_engines_with_a_dictionary_attached)."""
    t0 = time.time()
    got = H.run_legs(dict_vectors, show=lambda label, row: label in dict_vectors.CARRIERS)
    for name in ("general", "records", "scan", "gang8"):
        for label in dict_vectors.CARRIERS:
            assert got[name]["rows"][label][H.ENGINE] > 0, (name, label)
    assert got["gang8"]["gangs"] == [8, 8], got["gang8"]["gangs"]
    assert all(g <= 1 for g in got["general"]["gangs"]), got["general"]["gangs"]   # (no gangs)
    assert all(r[H.ENGINE] == 0 for r in got["norec"]["rows"].values())
    print("wall time %.1f s" % (time.time() - t0))


def _g_caps(e):
    """path_harness.limit_caps for the final copy, and the bytes round position 0's image: where the copy's source passes from the
    dictionary into the output"""
    n, before = (int(x[1:]) for x in e["label"].split("-")[1:3])
    start = e["size"] - n
    return sorted(set(H.limit_caps(e["size"], n)) | {start + before - 1, start + before, start + before + 1})


def _output_limits(pkg):
    n = 0
    for e, comp, d in dict_vectors.load():
        if e["label"].startswith("G-"):
            caps = _g_caps(e)
            assert caps[-1] == e["size"] + 1 and caps[0] == e["size"] - int(e["label"].split("-")[1][1:]) - 3
            results = H.in_batches(pkg, [comp] * len(caps), caps, [d] * len(caps), what=e["label"])
            assert [r.result for r in results][-3:] == [3, 1, 1], e["label"]
            n += 1
    assert n == 8
    return n


def test_output_limits_at_a_dictionary_copy(pkg):
    """G: streams of 300 commands that end in one copy out of the dictionary (n = 2, 40, 300, 3000, `before` inside n); out_cap at every
    byte from 3 in front of the copy to 1 behind it, for the long ones round every 16-byte boundary and round position 0's image.
    Once as the launch picks, once in a fresh process with BROTLI_AMD_NO_SCAN=1."""
    t0 = time.time()
    _output_limits(pkg)
    assert H.in_a_child("test_gpu_dict_paths", "_output_limits", {"BROTLI_AMD_NO_SCAN": "1"})[0] == 8
    print("wall time %.1f s" % (time.time() - t0))


def test_dictionary_streams_in_one_wave_blocks(pkg):
    """two of A's streams and two of C's replicated to 4 * CUs + 1 streams in one batch with their dictionaries, each dictionary the
    same object for all its streams (one upload each): more than four blocks a CU, which are blocks of one wave whatever the streams
    are"""
    t0 = time.time()
    by = {e["label"]: (e, c, d) for e, c, d in dict_vectors.load()}
    four = [by["A-matrix-D300-cf"], by["A-matrix-D17-ctx"], by["C-regimes-ctx"], by["C-edge-w10-D2500-cf"]]
    assert len({id(v[2]) for v in four}) == 4
    results, _ = H.blocks_a_cu(pkg, four)
    for i, r in enumerate(results):
        e = four[i % 4][0]
        assert [r.result, r.error_code, r.decoded_size] == e["oracle"] and [r.consumed, r.num_commands, r.num_metablocks] == e["success"], i
    print("wall time %.1f s" % (time.time() - t0))


_small = []


def _small_streams():
    """cut-down forms of at most 2000 bytes of output: A's first-command copies and the matrix for a dictionary of 17 bytes without its
    copies of more than 25 bytes, B's commands round the regimes' borders without the stretch that fills three windows, D's ring streams
    -> [(label, stream, output, dictionary)]"""
    if not _small:
        by = {e["label"]: (e, c, d) for e, c, d in dict_vectors.load()}
        for label in ("A-first-p0-d1-n65-mbend-cf", "A-first-p0-d16-n1040-mbend-cf", "A-first-p2-d17-n1040-last-cf", "A-first-p17-d33-n65-lits-ctx",
                      "D-w22-code5-zero+1", "D-w22-implicit-inside", "D-w10-code9-reach+1", "D-w10-code0-reach", "C-run-ctx"):
            e, c, d = by[label if label.endswith(("-cf", "-ctx")) else label + "-cf"]
            assert e["valid"] and e["size"] <= 2000, label
            _small.append((e["label"], c, dict_vectors.expected(c, e["size"], d)[1], d))
        made = [("A-matrix-D17-cut", [[c for c in M.a_matrix(17)[:-1] if c[1] <= 25] + [(2, 0, 0)]], 22, (1017, 17))]
        for size, target, what in ((600, 408, "copy"), (600, 408, "word"), (2500, 1, "copy"), (1009, 1007, "copy")):
            head, mid, _ = M.b_stream(size, target, what, 1)
            made.append(("B-D%d-p%d-%s-cut" % (size, target, what), [head, mid[:14] + [(2, 0, 0)]], M.B_WBITS, (2000 + size, size)))
        for label, blocks, wbits, dspec in made:
            d = dict_vectors.dictionary(*dspec)
            real = M.emit(blocks, "cf", wbits, d, literals=M.CV.LongLiterals(7))[3]
            for kind in ("cf", "ctx"):
                comp, raw, log, _ = M.emit(real, kind, wbits, d)
                assert len(raw) <= 2000 and any(r["distance"] > r["pos"] for r in log if r["coding"] != "tail"), (label, len(raw))   # (a copy out of the dictionary, or a word whose number it moves)
                assert dict_vectors.expected(comp, len(raw), d)[1] == raw
                _small.append((label + "-" + kind, comp, raw, d))
    return list(_small)


@pytest.mark.parametrize("chunks", [(1, 1), (3, 3), (65536, 1)])
def test_small_streams_byte_by_byte(pkg, chunks):
    """cut-down forms of A, B and D through a DecoderState with the dictionary attached: every byte, the final result, the totals of
    consumed and delivered bytes, and no call that delivers more than its room.  The calls are not compared one for one: the model
    of the reference's driver (stream_model.ReferenceStream) places its stops from the oracle's trace of a decode without a
    dictionary (brotli_oracle_decode_trace takes none), and a stream made for a dictionary does not decode without it -- giving the
    model the dictionary's effect takes a new entry point of the oracle, not a change of the model; the totals stay."""
    ic, oc = chunks
    t0 = time.time()
    for label, comp, raw, d in _small_streams():
        info = dict_vectors.expected(comp, len(raw), d)[0]
        got, out = H.product_seq(pkg, comp, ic, oc, d)
        assert got[-1][0] == sm.RESULT_SUCCESS and out == raw, (label, chunks, got[-1], len(out), len(raw))
        assert sum(g[1] for g in got) == info.consumed and sum(g[2] for g in got) == info.decoded_size == len(raw) and all(g[2] <= oc for g in got), (label, chunks)
    print("wall time %.1f s" % (time.time() - t0))


def test_four_dictionary_streams_in_a_stream_set(pkg):
    """four of the cut-down streams with chunks (64, 37): the states stepped by a StreamSet and the same four stepped alone give the
    same calls and bytes, and the bytes are the oracle's"""
    small = {s[0]: s for s in _small_streams()}
    names = ["A-matrix-D17-cut-ctx", "B-D600-p408-copy-cut-cf", "B-D2500-p1-copy-cut-ctx", "D-w10-code9-reach+1-cf"]
    jobs = [dict(data=small[n][1], ic=64, oc=37, lw=False, dict=small[n][3]) for n in names]
    H.stream_set_like_solo(pkg, jobs, names, [small[n][2] for n in names])
