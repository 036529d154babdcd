"""Every command symbol, every distance symbol and every shape of copy on every command path of the device (needs a real MI355X).

The kernels turn a command symbol into lengths and extra-bit fields in four places (kCmdLut of the checked loop, the lean loops,
the generated record run, the path engine's PE_TC), a distance symbol into a distance in at least five, and carry a copy out in
more than a dozen shapes -- by the command's lane, by big_item, staged through LDS, by levels of dependent copies, as a pattern
fill, held in registers across an exit.  An encoder library chooses which of these a stream meets.  The streams of
tests/golden/emitter_copies/ (tools/make_copy_vectors.py, pinned on the CPU by test_emitter_copies_cpu.py) hold every one by
construction; here they go through each path, against the oracle: result, error code, decoded size, every byte, and for
successes consumed, num_commands, num_metablocks."""
import hashlib
import random
import time

import pytest

import copy_vectors
import path_harness as H
import stream_model as sm

import make_copy_vectors as C  # noqa: I100  (tools/, which path_harness has put on the path)

pytestmark = pytest.mark.gpu


def test_every_vector_whole_short_truncated_and_damaged(pkg):
    """every stream of tests/golden/emitter_copies/ with exact, short, half, random and roomy output buffers and four truncated or
    bit-flipped copies each (path_harness.variants); those of more than 4 MiB of output -- S2 and the two window-24 forms of D --
    exact, one short, truncated and with one bit flipped; batches of at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2018)
    datas, caps = [], []
    for e, comp in copy_vectors.load():
        if e["size"] <= 1 << 22:
            d, c = H.variants(rnd, comp, e["size"])
        else:
            flipped = bytearray(comp); flipped[rnd.randrange(len(comp) // 2, len(comp))] ^= 1 << rnd.randrange(8)
            d, c = [comp, comp, comp[:rnd.randrange(len(comp) // 2, len(comp))], bytes(flipped)], [e["size"], e["size"] - 1, e["size"] + 64, e["size"] + 64]
        datas += d; caps += c
    H.in_batches(pkg, datas, caps, what="vectors")
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))


def test_the_streams_of_window_24_on_three_paths(pkg):
    """S2 (insert code 22 / 23, copy code 22 / 23 and 20 or 22 distance bits behind one another, 16 MB into the window) and D under
    (0, 0) and (3, 120) (every distance symbol up to 2^24 - 16): the general, records and checked legs.  They are kept out of the
    seven-leg test, which they made more than twice as slow as that of test_gpu_words.py."""
    t0 = time.time()
    got = H.run_legs(copy_vectors, "wide_set", [l for l in H.LEGS if l[0] in ("general", "records", "checked")])
    assert set(got) == {"general", "records", "checked"}
    print("wall time %.1f s" % (time.time() - t0))


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """copy_vectors.leg_set (two batches, each led by T's long form of more than 64 KiB, the size from which a launch forms gangs)
    in a fresh process per leg of path_harness.LEGS: the path engine's one-block form, whatever the launch picks, gangs of
    eight, the scan engine, the command records, the checked loop alone, and no records at all.  All legs return the same status
    words and SHA-256s, and those are the oracle's.  `engine_commands` says which path ran: T goes through the engine it is made
    for, under the bar test_gpu_words.py sets for its text-like vector; for the others the share is printed, and the general
    leg's must be above 0 for M and H."""
    t0 = time.time()
    got = H.run_legs(copy_vectors)
    # which path ran
    eng = lambda name, label: got[name]["rows"][label][H.ENGINE]
    cmds = lambda label: got["general"]["rows"][label][H.COMMANDS]
    for label in ("T-text-cf", "T2-text-long-cf"):
        assert eng("general", label) >= 0.9 * cmds(label), (label, eng("general", label), cmds(label))
        assert eng("default", label) > 0 and eng("gang8", label) > 0 and eng("scan", label) > 0, label
        assert eng("records", label) >= 0.9 * cmds(label), (label, eng("records", label), cmds(label))
    assert eng("scan", "T-text-cf4") > 0
    assert eng("records", "T-text-ctx") >= 0.9 * cmds("T-text-ctx"), (eng("records", "T-text-ctx"), cmds("T-text-ctx"))
    for label in ("M-rows-w22-cf", "M-mixed-w22-cf", "H-chains-cf"):
        assert eng("general", label) > 0, label
    assert got["gang8"]["gangs"] == [8, 8], got["gang8"]["gangs"]
    assert all(g <= 1 for g in got["general"]["gangs"]), got["general"]["gangs"]   # (no gangs)
    assert all(r[H.ENGINE] == 0 for r in got["norec"]["rows"].values())
    print("wall time %.1f s" % (time.time() - t0))


def _output_limits(pkg):
    n = 0
    for e, comp in copy_vectors.load():
        if e["label"].startswith("L-"):
            copy_len = int(e["label"].split("-")[1][1:])
            caps = H.limit_caps(e["size"], copy_len)
            assert caps[-1] == e["size"] + 1 and caps[0] == e["size"] - copy_len - 3
            results = H.in_batches(pkg, [comp] * len(caps), caps, what=e["label"])
            assert [r.result for r in results][-3:] == [3, 1, 1], e["label"]
            n += 1
    assert n == 24
    return n


def test_output_limits_at_a_copy(pkg):
    """L: streams of 3000 commands that end in one copy of each execution shape; out_cap at every byte around the copy's ends and,
    for the long ones, around every 16-byte boundary inside it (the checked loop clips the long shapes at out_cap and holds the
    short ones in registers across the exit).  Once as the launch picks, once in a fresh process with BROTLI_AMD_NO_SCAN=1."""
    t0 = time.time()
    _output_limits(pkg)
    assert H.in_a_child("test_gpu_copies", "_output_limits", {"BROTLI_AMD_NO_SCAN": "1"})[0] == 24
    print("wall time %.1f s" % (time.time() - t0))


def _small_streams():
    """the cut-down matrix, W at window 10 -- in less than the 1024 bytes of its ring buffer, and in 2000, which wrap it -- and one
    chain of depth 8, at most 2000 bytes of output each, CF and CTX -> [(label, stream, output)]"""
    out = []
    for label, cmds, wbits in (("M-small", C.m_small_commands(), 22), ("W-small", C.w_small_commands(False), 10), ("H-small", C.h_small_commands(), 22),
                               ("W-wraps", C.w_small_commands(True), 10)):
        real = C.realise([cmds], wbits, 170)
        for kind in ("cf", "ctx"):
            comp, raw, log, _ = C.emit(real, kind, wbits)
            assert len(raw) <= 2000
            out.append((label + "-" + kind, comp, raw))
    return out


@pytest.mark.parametrize("chunks", [(1, 1), (3, 3), (65536, 1)])
def test_small_streams_byte_by_byte(pkg, chunks):
    """cut-down forms of M, W and H through BrotliDecoderDecompressStream: call for call what the model of the reference's driver
    returns (tests/stream_model.py), and the oracle's bytes.  W at window 10 fits its ring buffer of 1024 bytes in the form that
    is compared call for call; the form of 2000 bytes wraps it, and for such streams the product's contract (include/brotli/decode.h,
    test_stream_contract.test_streaming_calls_where_the_ring_wraps) is every byte, the final result and the totals: it keeps no ring
    and stops for output only where the caller's buffer is full."""
    ic, oc = chunks
    for label, comp, raw in _small_streams():
        if label.startswith("W-wraps"):
            got, out = H.product_seq(pkg, comp, ic, oc)
            info = copy_vectors.expected(comp, len(raw), 0)[0]
            assert got[-1][0] == sm.RESULT_SUCCESS and out == raw, (label, chunks, got[-1])
            assert sum(g[2] for g in got) == info.decoded_size and sum(g[1] for g in got) == info.consumed and all(g[2] <= oc for g in got), (label, chunks)
            continue
        out = H.streamed_like_the_model(pkg, comp, ic, oc, label)
        assert out == copy_vectors.expected(comp, len(raw), 0)[1] == raw, label


def test_the_windows_edge_and_the_matrix_in_a_stream_set(pkg):
    """W at window 10 and M's window-16 form (NPOSTFIX 3, NDIRECT 120) with chunks (4096, 517): four states stepped by a StreamSet
    and the same four stepped alone give the same calls and bytes, and the bytes are the oracle's"""
    by = {e["label"]: (e, c) for e, c in copy_vectors.load()}
    names = ["W-edge-w10-cf", "W-edge-w10-ctx", "M-rows-w16-cf", "M-mixed-w16-ctx"]
    jobs = [dict(data=by[n][1], ic=4096, oc=517, lw=False) for n in names]
    want = [copy_vectors.expected(by[n][1], by[n][0]["size"], 0)[1] for n in names]
    assert [hashlib.sha256(exp).hexdigest() for exp in want] == [by[n][0]["sha256"] for n in names]
    H.stream_set_like_solo(pkg, jobs, names, want)


def test_the_matrix_with_custom_dictionaries(pkg):
    """the cut-down matrix emitted for custom dictionaries of 1, 15, 16, 17, 300 and 70000 bytes: every copy starts 1 .. 20 bytes
    inside the dictionary's end and runs over into the output, the first ones overlap themselves as well (cdict_copy splits at a
    distance of 16).  Against brotli_oracle_decode_dict through path_harness.check, CF and CTX, whole, short and cut."""
    rnd = random.Random(301)
    datas, caps, dicts = [], [], []
    for size in (1, 15, 16, 17, 300, 70000):
        dictionary = bytes(rnd.choice(b"etaoin shrdlu,.\n") for _ in range(size))
        real = C.realise([C.m_dict_commands(size)], 22, 171, dictionary=dictionary)
        first = None
        for kind in ("cf", "ctx"):
            comp, raw, log, _ = C.emit(real, kind, 22, dictionary=dictionary)
            assert first in (None, raw)
            first = raw
            copies = [r for r in log if r["coding"] != "tail"]
            assert all(1 <= r["distance"] - r["pos"] <= min(20, size) and r["max_distance"] == r["pos"] + size for r in copies)
            assert {r["distance"] - r["pos"] for r in copies} == set(range(1, min(20, size) + 1))
            assert any(r["copy_len"] > r["distance"] for r in copies) and (size < 16 or any(r["copy_len"] > r["distance"] - r["pos"] >= 16 for r in copies))
            info, out = H.expected(comp, len(raw), 0, dictionary)
            assert info.result == 1 and out == raw
            for cap in (len(raw), len(raw) - 1, len(raw) // 2, len(raw) + 1000):
                datas.append(comp); caps.append(cap); dicts.append(dictionary)
            datas.append(comp[:len(comp) * 2 // 3]); caps.append(len(raw)); dicts.append(dictionary)
    H.check(pkg, datas, caps, dicts, flags=0, what="M with custom dictionaries")


def test_the_matrix_and_the_symbols_in_one_wave_blocks(pkg):
    """M and S1 replicated to 4 * CUs + 1 streams in one batch: more than four blocks a CU, which are blocks of one wave whatever
    the streams are; status words and every byte against the oracle, whose bytes have the manifest's SHA-256"""
    by = {e["label"]: (e, c) for e, c in copy_vectors.load()}
    four = [by["M-rows-w22-cf"], by["M-mixed-w22-ctx"], by["S1a-symbols-ctx"], by["S1b-symbols-cf"]]
    for e, c in four:
        assert hashlib.sha256(copy_vectors.expected(c, e["size"], 0)[1]).hexdigest() == e["sha256"]
    results, _ = H.blocks_a_cu(pkg, four)
    for i, r in enumerate(results):
        e = four[i % 4][0]
        assert (r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands, r.num_metablocks) == (1, 1, e["size"], e["csize"], e["commands"], e["metablocks"]), i
