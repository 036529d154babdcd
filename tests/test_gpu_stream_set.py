"""Stream sets on a real MI355X (include/brotli/batch.h: BrotliAmdStreamSetDecompress): many streaming states stepped by one launch.

What is expected never comes from the set itself: call for call from the model of the reference's driver (tests/stream_model.py:
ReferenceStream) and byte for byte from the oracle where the model covers the stream; for the streams it does not cover -- those that
wrap their ring, damaged ones, dictionaries -- from BrotliDecoderDecompressStream on a fresh state stepped alone on the same schedule,
which the stream set does not change.

The states of a run are driven in lockstep, each by run_schedule's rule (stream_model.run_schedule, the loop of the reference's
src/bin/integration_tests.rs:122-216): new input only after NEEDS_MORE_INPUT with nothing pending, calls without input at the end while
they still deliver something.  A state whose schedule is over STAYS in the calls that follow, with no input, and has to go on answering
what the solo function answers such a state: its last result again, nothing consumed, nothing written."""
import ctypes
import os
import random

import numpy as np
import pytest

import oracle_lib as oracle
import stream_model as sm
from conftest import ROOT
from test_stream_contract import SMALL, WRAP

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "testdata")
TINY = ["10x10y.compressed", "64x.compressed", "ukkonooa.compressed", "monkey.compressed", "xyzzy.compressed", "quickfox.compressed",
        "random1024.br", "x.compressed.03"]   # decode to at most 1024 bytes


def _data(name):
    return open(os.path.join(GOLD, name), "rb").read()


_oracle = {}


def _expected(data, flags=1):
    """the oracle's (info, bytes) of a stream, computed once"""
    key = (data, flags)
    if key not in _oracle:
        _oracle[key] = oracle.decode(data, 1 << 22, flags)
    return _oracle[key]


class Run:
    """n states and their schedules.  jobs: [(data, in_chunk, out_chunk)] or dicts with data / ic / oc / lw / dict.
    how(round) -> "set" or "solo": the whole round through one BrotliAmdStreamSetDecompress, or state by state through
    BrotliDecoderDecompressStream."""

    def __init__(self, pkg, jobs, max_states=None):
        self.pkg, self.L = pkg, pkg.load_library()
        jobs = [j if isinstance(j, dict) else dict(data=j[0], ic=j[1], oc=j[2]) for j in jobs]
        self.jobs, self.n = jobs, len(jobs)
        n = self.n
        self.states = [pkg.DecoderState(large_window=j.get("lw", True), dictionary=j.get("dict")) for j in jobs]
        self.set = pkg.StreamSet(max_states or n)
        self.src = [ctypes.create_string_buffer(j["data"], max(1, len(j["data"]))) for j in jobs]
        self.outb = [ctypes.create_string_buffer(max(1, j["oc"])) for j in jobs]
        self.base = [ctypes.addressof(b) for b in self.src]
        self.oaddr = [ctypes.addressof(b) for b in self.outb]
        self.st = (ctypes.c_void_p * n)(*[s._h for s in self.states])
        self.ai, self.ao, self.tot = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        self.ni, self.no = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()   # (addresses)
        self.res = (ctypes.c_int * n)()
        self.solo = self.L["BrotliDecoderDecompressStream"]   # (addresses of the arrays' entries: a prototype of plain pointers)
        self.solo.argtypes = [ctypes.c_void_p] * 6
        self.seq = [[] for _ in range(n)]      # per state: (result, consumed, produced) of every call of its schedule
        self.out = [[] for _ in range(n)]
        self.calls = []                         # per set call: (bytes of input given, launches, transfers)

    def close(self):
        self.set.close()
        for s in self.states:
            s.close()

    def bytes_of(self, i):
        return b"".join(self.out[i])

    def run(self, how=lambda k: "set", extra=2, max_rounds=400000):
        n, jobs, L = self.n, self.jobs, self.L
        ai, ao, ni, no, res = self.ai, self.ao, self.ni, self.no, self.res
        size = [len(j["data"]) for j in jobs]
        ic, oc = [j["ic"] for j in jobs], [j["oc"] for j in jobs]
        pos, p_off, p_len, result = [0] * n, [0] * n, [0] * n, [2] * n
        ao_np, no_np = np.ctypeslib.as_array(ao), np.ctypeslib.as_array(no)
        ai_np, res_np = np.ctypeslib.as_array(ai), np.ctypeslib.as_array(res)
        oc_np, oaddr_np = np.array(oc, dtype=ao_np.dtype), np.array(self.oaddr, dtype=no_np.dtype)
        live, over = list(range(n)), np.zeros(n, dtype=bool)
        want_res = np.zeros(n, dtype=res_np.dtype)
        for k in range(max_rounds):
            nxt = []
            for i in live:
                if p_len[i] == 0 and result[i] == 2:
                    if pos[i] >= size[i]:
                        if not (self.seq[i] and self.seq[i][-1][2] != 0):
                            over[i] = True; want_res[i] = 2
                            continue
                    else:
                        p_off[i] = pos[i]; p_len[i] = min(ic[i], size[i] - pos[i]); pos[i] += p_len[i]
                ai[i] = p_len[i]; ni[i] = self.base[i] + p_off[i]
                nxt.append(i)
            live = nxt
            if not live:
                extra -= 1
                if extra < 0:
                    break
            ai_np[over] = 0
            ao_np[:] = oc_np; no_np[:] = oaddr_np
            given = [p_len[i] for i in live]
            if how(k) == "set":
                assert L.BrotliAmdStreamSetDecompress(self.set._h, n, self.st, ai, ni, ao, no, self.tot, res) == 0, self.pkg.last_error()
                self.calls.append((sum(given), self.set.last_launches(), self.set.last_transfers()))
            else:
                for i in range(n):
                    o = 8 * i
                    res[i] = self.solo(self.st[i], ctypes.addressof(ai) + o, ctypes.addressof(ni) + o, ctypes.addressof(ao) + o,
                                       ctypes.addressof(no) + o, ctypes.addressof(self.tot) + o)
            # the states whose schedule is over: their last result again, nothing consumed, nothing written
            if over.any():
                assert (res_np[over] == want_res[over]).all() and (ao_np[over] == oc_np[over]).all() and (ai_np[over] == 0).all(), \
                    (k, [(i, int(res_np[i]), int(want_res[i])) for i in np.flatnonzero(over) if res_np[i] != want_res[i]][:5])
            for i, g in zip(live, given):
                used, made, r = g - ai[i], oc[i] - ao[i], res[i]
                self.seq[i].append((r, used, made))
                if made:
                    self.out[i].append(ctypes.string_at(self.oaddr[i], made))
                p_off[i] += used; p_len[i] -= used; result[i] = r
                if r in (0, 1):
                    over[i] = True; want_res[i] = r
            live = [i for i in live if not over[i]]
        else:
            raise AssertionError("schedules did not end")
        return self


def _model(data, ic, oc):
    m = sm.ReferenceStream(data)
    return sm.run_schedule(lambda pending, cap: m.call(len(pending), cap), data, ic, oc, drain=True)


def _first_diff(got, want):
    return next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("chunks", [(65536, 65536), (3, 3), (12, 1), (1, 65536)])
def test_twelve_states_call_for_call_against_the_model(pkg, chunks, cut):
    """one state per fixture of test_stream_contract.SMALL, whole or cut to two thirds, all in every call: every state's sequence of
    (result, consumed, produced) is the model's and its bytes are the oracle's.  They finish at different calls -- after one, after a
    hundred thousand -- and stay in the calls that follow."""
    ic, oc = chunks
    datas = [_data(n) for n in SMALL]
    if cut:
        datas = [d[: max(1, len(d) * 2 // 3)] for d in datas]
    run = Run(pkg, [(d, ic, oc) for d in datas]).run()
    try:
        for i, (name, d) in enumerate(zip(SMALL, datas)):
            want = _model(d, ic, oc)
            assert run.seq[i] == want, (name, len(d), chunks, _first_diff(run.seq[i], want))
            assert run.bytes_of(i) == _expected(d)[1], name
        # they do finish at different calls: by the model the schedules of the twelve have 2 distinct lengths when a chunk holds a
        # whole fixture ({1, 3} whole, {1, 2} cut) and 6 to 12 under the small chunkings
        assert len({len(s) for s in run.seq}) > (1 if ic == 65536 else 3)
    finally:
        run.close()


def _solo_twin(pkg, jobs):
    return Run(pkg, jobs).run(how=lambda k: "solo")


def _same_as_solo(run, twin, names):
    for i, name in enumerate(names):
        assert run.seq[i] == twin.seq[i], (name, _first_diff(run.seq[i], twin.seq[i]))
        assert run.bytes_of(i) == twin.bytes_of(i), name
        a, b = run.states[i], twin.states[i]
        assert (a.error_code(), a.error_string(), a.is_finished(), a.is_used(), a.has_more_output()) == \
               (b.error_code(), b.error_string(), b.is_finished(), b.is_used(), b.has_more_output()), name


def test_a_set_of_one_is_the_solo_call(pkg):
    jobs = [(_data("alice29.txt.compressed"), 4096, 517)]
    run, twin = Run(pkg, jobs).run(), _solo_twin(pkg, jobs)
    try:
        _same_as_solo(run, twin, ["alice29"])
        assert run.seq[0][-1][0] == 1 and run.bytes_of(0) == _expected(jobs[0][0])[1]
        assert run.seq[0] == _model(jobs[0][0], 4096, 517)
        assert all((l, t) == (0, 0) for g, l, t in run.calls if not g) and any(l for g, l, t in run.calls)
    finally:
        run.close(); twin.close()


@pytest.mark.parametrize("chunks", [(4096, 517), (65536, 1000)])
def test_streams_that_wrap_their_ring_and_errors_beside_healthy_ones(pkg, chunks):
    """the WRAP fixtures, borked.compressed and a fixture with one flipped bit among healthy streams: every state's call sequence, bytes,
    error code and error string are those of a fresh state stepped alone on the same schedule; totals and bytes are the oracle's where
    the stream is valid.  An error in one state changes nothing for the others."""
    ic, oc = chunks
    rnd = random.Random(517)
    alice = _data("alice29.txt.compressed")
    flipped = bytearray(alice); flipped[rnd.randrange(len(alice) // 2, len(alice))] ^= 1 << rnd.randrange(8)
    named = [(n, _data(n)) for n in WRAP] + [("borked.compressed", _data("borked.compressed")), ("alice29 with a flipped bit", bytes(flipped)),
                                             ("alice29", alice), ("quickfox", _data("quickfox.compressed")), ("monkey", _data("monkey.compressed"))]
    jobs = [(d, ic, oc) for _, d in named]
    run, twin = Run(pkg, jobs).run(), _solo_twin(pkg, jobs)
    try:
        _same_as_solo(run, twin, [n for n, _ in named])
        errors = 0
        for i, (name, d) in enumerate(named):
            info, exp = _expected(d)
            if info.result == 1:
                assert run.seq[i][-1][0] == 1 and run.bytes_of(i) == exp, name
                assert sum(s[2] for s in run.seq[i]) == info.produced and sum(s[1] for s in run.seq[i]) == info.consumed, name
            else:
                errors += run.seq[i][-1][0] == 0
                # (a damaged stream: the oracle decodes it in one piece and delivers nothing, a streaming state has handed over what earlier
                # chunks decoded to -- its bytes were compared with the solo twin's above)
                assert run.states[i].error_code() == info.error_code, (name, run.states[i].error_code(), info.error_code)
        assert errors == 2
    finally:
        run.close(); twin.close()


def test_mixed_phases_in_one_call(pkg):
    """one call holds a fresh state, one mid-stream, one finished, one with a latched error, one given no input, one that owes output and is
    given no room (NEEDS_MORE_OUTPUT, nothing consumed), one with large_window off on a large-window stream, and one with a dictionary: each
    answers what its twin -- the same history, stepped alone -- answers, in that call and in the ones that follow."""
    import dict_streams as ds
    alice, quick = _data("alice29.txt.compressed"), _data("quickfox.compressed")
    _, dcomp, ddict, dexp = ds.vectors()[0]
    lw_stream = b"\x11\xd8"   # the large-window header (WBITS 24) and an empty last metablock
    assert _expected(lw_stream, 1)[0].result == 1 and _expected(lw_stream, 0)[0].result == 0

    def history():
        s = dict(fresh=pkg.DecoderState(large_window=True), mid=pkg.DecoderState(large_window=True), finished=pkg.DecoderState(large_window=True),
                 failed=pkg.DecoderState(large_window=True), idle=pkg.DecoderState(large_window=True), owing=pkg.DecoderState(large_window=True),
                 small_window=pkg.DecoderState(large_window=False), with_dict=pkg.DecoderState(large_window=True, dictionary=ddict))
        assert s["mid"].decompress_stream(alice[:4096], 1 << 16)[0] == 2
        assert s["finished"].decompress_stream(quick, 4096)[0] == 1
        assert s["failed"].decompress_stream(_data("borked.compressed"), 4096)[0] == 0
        assert s["owing"].decompress_stream(quick, 5) == (3, len(quick), _expected(quick)[1][:5])
        return s
    calls = [
        dict(fresh=(alice[:4096], 1 << 16), mid=(alice[4096:8192], 1 << 16), finished=(b"more", 64), failed=(b"more", 64), idle=(b"", 64),
             owing=(b"xyz", 0), small_window=(lw_stream, 64), with_dict=(dcomp, 1 << 16)),
        dict(fresh=(alice[4096:], 1 << 18), mid=(alice[8192:], 1 << 18), finished=(b"", 64), failed=(b"", 64), idle=(quick, 64),
             owing=(b"xyz", 7), small_window=(b"", 64), with_dict=(b"", 64)),
        dict(fresh=(b"", 64), mid=(b"", 64), finished=(b"", 64), failed=(b"", 64), idle=(b"", 64), owing=(b"", 1 << 10), small_window=(b"", 64),
             with_dict=(b"", 64)),
    ]
    a, b = history(), history()
    names = list(a)
    sset = pkg.StreamSet(len(names))
    try:
        got_all = []
        for call in calls:
            got = sset.decompress([a[k] for k in names], [call[k][0] for k in names], [call[k][1] for k in names])
            want = [b[k].decompress_stream(*call[k]) for k in names]
            for k, g, w in zip(names, got, want):
                assert g == w, (k, g[:2], len(g[2]), w[:2], len(w[2]))
                assert (a[k].error_code(), a[k].error_string(), a[k].is_finished(), a[k].is_used(), a[k].has_more_output()) == \
                       (b[k].error_code(), b[k].error_string(), b[k].is_finished(), b[k].is_used(), b[k].has_more_output()), k
            got_all.append(dict(zip(names, got)))
        first, second, third = got_all
        assert sset.last_launches() == 0     # (the third call: nobody had input)
        assert first["owing"] == (3, 0, b"") and first["finished"] == (1, 0, b"") and first["failed"] == (0, 0, b"") and first["idle"] == (2, 0, b"")
        assert first["small_window"][0] == 0 and a["small_window"].error_code() == _expected(lw_stream, 0)[0].error_code
        assert first["with_dict"] == (1, len(dcomp), dexp)
        exp_alice, exp_quick = _expected(alice)[1], _expected(quick)[1]
        assert first["fresh"][2] + second["fresh"][2] == exp_alice and second["fresh"][0] == 1
        assert first["mid"][2] + second["mid"][2] == exp_alice[len(exp_alice) - len(first["mid"][2] + second["mid"][2]):] and second["mid"][0] == 1
        assert second["owing"] == (3, 0, exp_quick[5:12]) and third["owing"] == (1, 0, exp_quick[12:])
        assert second["idle"] == (1, len(quick), exp_quick) and third["idle"] == (1, 0, b"")   # (43 bytes: they fit the 64 it was given)
    finally:
        sset.close()
        for s in list(a.values()) + list(b.values()):
            s.close()


def test_a_state_goes_from_the_set_to_solo_calls_and_back(pkg):
    """chunk by chunk alternately through the set and alone: one sequence of calls, the model's, and the oracle's bytes"""
    names = ["alice29.txt.compressed", "monkey.compressed", "random1024.br"]
    jobs = [(_data("alice29.txt.compressed"), 1000, 3000), (_data("monkey.compressed"), 7, 5), (_data("random1024.br"), 12, 65536)]
    run = Run(pkg, jobs).run(how=lambda k: "set" if k % 2 == 0 else "solo")
    try:
        for i, (name, (d, ic, oc)) in enumerate(zip(names, jobs)):
            want = _model(d, ic, oc)
            assert run.seq[i] == want, (name, _first_diff(run.seq[i], want))
            assert run.bytes_of(i) == _expected(d)[1], name
        assert sum(l for _, l, _ in run.calls) > 20
    finally:
        run.close()


def test_one_launch_and_two_transfers_a_call(pkg):
    """64 states over fixtures that decode to at most 1024 bytes: every call in which some state had input is ONE launch and at most two
    copies of payload between host and device -- the solo loop's 64 launches and 128 copies --, and a call in which none had is none."""
    jobs = [(_data(TINY[i % len(TINY)]), (5, 16, 97, 4096)[(i // len(TINY)) % 4], 64 if i % 3 else 4096) for i in range(64)]
    run = Run(pkg, jobs).run()
    try:
        for i, (d, ic, oc) in enumerate(jobs):
            assert run.seq[i][-1][0] == 1 and run.bytes_of(i) == _expected(d)[1], i
            assert run.seq[i] == _model(d, ic, oc), i
        with_input = [c for c in run.calls if c[0]]
        without = [c for c in run.calls if not c[0]]
        assert len(with_input) > 100 and without
        assert all(l == 1 and t <= 2 for _, l, t in with_input), [c for c in with_input if c[1] != 1 or c[2] > 2][:5]
        assert all((l, t) == (0, 0) for _, l, t in without)
        assert any(t == 2 for _, _, t in with_input)
    finally:
        run.close()


def test_growth_launches_again_the_states_that_grow_alone(pkg):
    """zeros.compressed -- 13 bytes that decode to 256 KiB, past the first 64 KiB device output buffer -- beside eight alice29 states: the call
    that feeds it launches more than once, and no state is decoded twice for it: the commands the device decoded for every state stay within
    the streaming bound of test_streaming_goes_on_inside_a_metablock."""
    alice, zeros = _data("alice29.txt.compressed"), _data("zeros.compressed")
    jobs = [(zeros, 65536, 65536)] + [(alice, 4096, 65536)] * 8
    run = Run(pkg, jobs).run()
    try:
        assert run.calls[0][1] >= 2
        assert all((l >= 1) if g else (l, t) == (0, 0) for g, l, t in run.calls)
        for i, (d, _, _) in enumerate(jobs):
            info, exp = _expected(d)
            assert run.seq[i][-1][0] == 1 and run.bytes_of(i) == exp, i
            calls = len(run.seq[i])
            assert info.num_commands <= run.states[i].device_commands() <= 2 * info.num_commands + 64 * calls, \
                (i, info.num_commands, run.states[i].device_commands(), calls)
    finally:
        run.close()


@pytest.mark.parametrize("shape", ["eight waves", "four waves", "one wave"])
def test_block_shapes_the_solo_call_never_uses(pkg, shape):
    """more states than compute units: cus + 44, 2 cus + 88, 4 cus + 76 of them (300, 600, 1100 on 256 CUs) make launches of eight-, four- and
    one-wave blocks, shapes a launch of one stream never has.  The small fixtures are fed 7 bytes a round and alice29 1500, so from the second
    round on the descriptors are resumed ones, most of them inside a metablock (BrotliAmdResume: mid_valid).  Bytes and final results are
    the oracle's."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = {"eight waves": cus + 44, "four waves": 2 * cus + 88, "one wave": 4 * cus + 76}[shape]
    alice = _data("alice29.txt.compressed")
    kinds = [(_data(name), 7, 16384) for name in TINY] + [(alice, 1500, 16384)] * 4
    jobs = [kinds[i % len(kinds)] for i in range(n)]
    run = Run(pkg, jobs).run(extra=0)
    try:
        bad = [i for i, (d, _, _) in enumerate(jobs) if run.seq[i][-1][0] != 1 or run.bytes_of(i) != _expected(d)[1]]
        assert not bad, (len(bad), [(i, len(jobs[i][0]), run.seq[i][-1], len(run.bytes_of(i))) for i in bad[:5]])
        assert all((l >= 1) if g else (l, t) == (0, 0) for g, l, t in run.calls)
    finally:
        run.close()


@pytest.mark.parametrize("chunks", [(12345, 181), (65536, 65536)])
def test_gangs_with_resumed_streams(pkg, chunks):
    """three states over streams of more than 64 KiB compressed each: few streams, long ones -- the planner may give each a gang of blocks,
    and from the second call on the gangs' streams are resumed ones.  Bytes and totals are the oracle's."""
    names = ["lcet10.txt.compressed", "plrabn12.txt.compressed", "mapsdatazrh.compressed"]
    jobs = [(_data(n), chunks[0], chunks[1]) for n in names]
    run = Run(pkg, jobs).run()
    try:
        for i, name in enumerate(names):
            info, exp = _expected(jobs[i][0])
            assert run.seq[i][-1][0] == 1 and run.bytes_of(i) == exp, name
            assert sum(s[2] for s in run.seq[i]) == info.produced and sum(s[1] for s in run.seq[i]) == info.consumed, name
            assert all(s[2] <= chunks[1] for s in run.seq[i])
    finally:
        run.close()


def test_streams_sent_back_unread_go_on_from_their_boundary(pkg):
    """More states than compute units, few enough for engine blocks, most of them the engines' kind (long copies) and a quarter text: the launch
    gives the engines' streams blocks of sixteen waves and sends the texts back unread, to a launch of small blocks behind it
    (BROTLI_AMD_FLAG_DEFER).  A stream sent back reports no boundary; one that came RESUMED has to go on from the boundary it came with -- not from
    byte 0, which a streaming state's trimmed buffers no longer hold (lcet10 has more than 64 KiB compressed: its input is trimmed on the way).
    The smallest case of a resumed stream in a shape a launch of one stream never has that went wrong: bytes and results are the oracle's, and
    no state's commands are decoded again (the streaming bound of test_streaming_goes_on_inside_a_metablock)."""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import workloads as w
    if not w.encoder_available():
        pytest.skip("no encoder library: no streams of the engines' kind")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    raws = [w.long_backref_stream(900 + k, 1 << 20) for k in range(3)]
    engines = [w.brotli_compress(r, 5, 22) for r in raws]
    for c, r in zip(engines, raws):
        _oracle[(c, 1)] = oracle.decode(c, len(r) + 64, 1)
        assert _oracle[(c, 1)][1] == r
    lcet = _data("lcet10.txt.compressed")
    jobs = [((engines[i % 3], 16384, 1 << 18) if i % 4 else (lcet, 16384, 1 << 18)) for i in range(cus + 44)]
    run = Run(pkg, jobs).run(extra=0)
    try:
        for i, (d, _, _) in enumerate(jobs):
            info, exp = _expected(d)
            assert run.seq[i][-1][0] == 1 and run.bytes_of(i) == exp, (i, run.seq[i][-1], len(run.bytes_of(i)), len(exp))
            calls = len(run.seq[i])
            assert info.num_commands <= run.states[i].device_commands() <= 2 * info.num_commands + 64 * calls, \
                (i, info.num_commands, run.states[i].device_commands(), calls)
    finally:
        run.close()
