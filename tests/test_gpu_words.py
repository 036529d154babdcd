"""Every word of the static dictionary and every ring distance code on every command path of the device (needs a real MI355X).

Four places in the kernel turn a distance beyond the maximum distance into a word, four resolve the short distance codes --
the checked loop (process_commands), the command records of context-modelled metablocks (lean_rec_commands), the path
engine's passes (path_engine<true, false>, pe_dict_word) and the forms that stop in front of a word and hand the command
over (the lean form, the gangs' form, scan_engine) -- and an encoder library writes a handful of the 121 transforms, no word of
zero or one byte, no ring code that names a word and no invalid reference.  The streams of tests/golden/emitter_words/
(tools/make_word_vectors.py, pinned on the CPU by test_emitter_words_cpu.py) do; here they go through each of those paths,
against the oracle: result, error code, decoded size, every byte, and for successes consumed, num_commands, num_metablocks."""
import hashlib
import random
import time

import pytest

import oracle_lib as oracle
import path_harness as H
import word_vectors

pytestmark = pytest.mark.gpu


def test_every_vector_whole_short_truncated_and_damaged(pkg):
    """every stream of tests/golden/emitter_words/: the valid ones with exact, short, half, random and roomy output buffers and
    four truncated or bit-flipped copies each, the invalid ones as they are; batches of at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2017)
    datas, caps = [], []
    for e, comp in word_vectors.load():
        if e["valid"]:
            d, c = H.variants(rnd, comp, e["size"])
            datas += d; caps += c
        else:
            datas += [comp, comp]; caps += [e["size"] + 64, max(0, e["size"] - 1)]
    H.in_batches(pkg, datas, caps, what="vectors")
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """The same 61 streams (word_vectors.leg_set: two batches of about 30, each with one stream of more than 64 KiB, the size
    from which a launch forms gangs) in a fresh process per leg (path_harness.LEGS): the path engine's one-block form with the words
    inside its passes (BROTLI_AMD_GANG=0), whatever the launch picks, gangs of eight, the scan engine, the command records
    (BROTLI_AMD_NO_SCAN=1), and the checked loop alone (plus BROTLI_AMD_ENGINE=norecall: no records for metablocks without context;
    =norec: none at all).  All legs return the same status words and SHA-256s, and those are the oracle's.  `engine_commands` says
    which path ran (csrc/brotli_device_abi.h: commands a command engine took; the record loop's commands count as well,
    brotli_kernels.hip, `engine_commands += took_` behind lean_rec_commands): the text-like vector C goes through the engine it is
    meant for."""
    t0 = time.time()
    got = H.run_legs(word_vectors, show=lambda label, row: label in ("C-text-cf", "C-text-ctx", "C-text-cf4", "C2-text-long-cf"))
    # which path ran
    eng = lambda name, label: got[name]["rows"][label][H.ENGINE]
    cmds = lambda label: got["general"]["rows"][label][H.COMMANDS]
    for label in ("C-text-cf", "C2-text-long-cf"):
        assert eng("general", label) >= 0.9 * cmds(label), (label, eng("general", label), cmds(label))   # (the words went out inside passes)
        assert eng("default", label) > 0 and eng("gang8", label) > 0 and eng("scan", label) > 0, label
        assert eng("records", label) >= 0.9 * cmds(label), (label, eng("records", label), cmds(label))
    assert eng("scan", "C-text-cf4") > 0
    assert eng("records", "C-text-ctx") >= 0.9 * cmds("C-text-ctx"), (eng("records", "C-text-ctx"), cmds("C-text-ctx"))
    assert got["gang8"]["gangs"] == [8, 8], got["gang8"]["gangs"]
    assert all(g <= 1 for g in got["general"]["gangs"]), got["general"]["gangs"]   # (no gangs)
    assert all(r[H.ENGINE] == 0 for r in got["norec"]["rows"].values())
    assert all(r[H.ENGINE] == 0 for l, r in got["checked"]["rows"].items() if "-ctx" not in l)   # (norecall leaves the context-modelled metablocks their records)
    print("wall time %.1f s" % (time.time() - t0))


def test_ring_codes_that_name_words(pkg):
    """E: short codes against the initial ring at P = 0, 1, 2, 3, 5, 12 and codes 4 .. 15 that land one to three beyond P --
    words named by a ring code, which push nothing --, and the same with copy lengths 2, 3 and 25 (ERROR_DICTIONARY);
    every one whole, one byte short of output, and cut after each of its bytes from the fourth on"""
    datas, caps = [], []
    for e, comp in word_vectors.load():
        if e["label"].startswith("E-"):
            datas += [comp, comp]; caps += [e["size"] if e["valid"] else e["size"] + 64, max(0, e["size"] - 1)]
            if e["csize"] < 64:
                for cut in range(4, len(comp)):
                    datas.append(comp[:cut]); caps.append(e["size"] + 64)
    assert len(datas) >= 180
    H.in_batches(pkg, datas, caps, what="ring codes that name words")


def test_output_limits_at_a_final_word(pkg):
    """G: streams of 3000 commands that end in a word of one byte, of two bytes, and in a three-byte-UTF-8 uppercase-all word
    with prefix and suffix; out_cap at every byte from 3 in front of the word to 1 behind it (the checked loop clips a word at
    the output limit, with a case of its own for a word of one byte)"""
    n = 0
    vectors = word_vectors.load()
    base = next(e["size"] for e, _ in vectors if e["label"] == "G-total1-cf") - 1  # (the three streams differ in their last command alone)
    for e, comp in vectors:
        if not e["label"].startswith("G-"):
            continue
        total = e["size"] - base
        assert total == {"total1": 1, "total2": 2}.get(e["label"].split("-")[1], total) and 1 <= total <= 40
        caps = list(range(e["size"] - total - 3, e["size"] + 2))
        results = H.check(pkg, [comp] * len(caps), caps, None, 0, e["label"])
        assert [r.result for r in results][-2:] == [1, 1] and results[-3].result == 3
        n += 1
    assert n == 6


@pytest.mark.parametrize("chunks", [(1, 1), (3, 3), (65536, 1)])
def test_small_streams_byte_by_byte(pkg, chunks):
    """H (at most 600 bytes of output, 30 words) through BrotliDecoderDecompressStream: call for call what the model of the
    reference's driver returns (tests/stream_model.py), as test_stream_contract.py does for the fixtures"""
    n = 0
    for e, comp in word_vectors.load():
        if e["label"].startswith("H-"):
            out = H.streamed_like_the_model(pkg, comp, *chunks, e["label"])
            assert out == word_vectors.expected(comp, e["size"], 0)[1] and hashlib.sha256(out).hexdigest() == e["sha256"]
            n += 1
    assert n == 2


def test_small_streams_with_custom_dictionaries(pkg):
    """H's command list emitted again for custom dictionaries of 1, 300 and 70000 bytes: the maximum distance grows by the
    dictionary's size and every word's number with it.  Against brotli_oracle_decode_dict, through the batch call of the
    custom-dictionary tests (path_harness.check); without its dictionary such a stream does not decode to the same bytes."""
    import make_word_vectors as M
    rnd = random.Random(300)
    cmds = M.h_commands()
    plain = M.emit(cmds, "cf", 22)[1]
    datas, caps, dicts = [], [], []
    for size in (1, 300, 70000):
        dictionary = bytes(rnd.choice(b"etaoin shrdlu,.\n") for _ in range(size))
        for kind in ("cf", "ctx"):
            comp, raw, log, _ = M.emit(cmds, kind, 22, dictionary=dictionary)
            assert raw == plain and sum(1 for r in log if r["word"]) >= 30 and all(r["max_distance"] == r["pos"] + size for r in log if r["word"])
            info, out = H.expected(comp, len(raw), 0, dictionary)
            assert info.result == 1 and out == raw
            assert oracle.decode(comp, len(raw), 0)[1] != raw
            for cap in (len(raw), len(raw) - 1, len(raw) // 2, len(raw) + 1000):
                datas.append(comp); caps.append(cap); dicts.append(dictionary)
            datas.append(comp[:len(comp) * 2 // 3]); caps.append(len(raw)); dicts.append(dictionary)
    H.check(pkg, datas, caps, dicts, flags=0, what="H with custom dictionaries")


def test_the_matrix_in_one_wave_blocks(pkg):
    """A/CF and A/CTX replicated to 4 * CUs + 1 streams in one batch: more than four blocks a CU, which are blocks of one wave
    whatever the streams are; status words and every byte against the oracle, whose bytes have the manifest's SHA-256"""
    by = {e["label"]: (e, c) for e, c in word_vectors.load()}
    four = [by["A1-matrix-cf"], by["A1-matrix-ctx"], by["A2-multibyte-cf"], by["A2-multibyte-ctx"]]
    for e, c in four:
        assert hashlib.sha256(word_vectors.expected(c, e["size"], 0)[1]).hexdigest() == e["sha256"]
    results, _ = H.blocks_a_cu(pkg, four)
    for i, r in enumerate(results):
        e = four[i % 4][0]
        assert (r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands, r.num_metablocks) == (1, 1, e["size"], e["csize"], e["commands"], e["metablocks"]), i
