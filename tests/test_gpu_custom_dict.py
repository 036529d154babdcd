"""Custom (LZ77 prefix) dictionaries on the device against the CPU oracle (brotli_oracle_decode_dict), through the C ABI: the
batch entry points BrotliAmdBatchDecodeHostDict / BrotliAmdBatchDecodeDeviceDict, BrotliAmdDecoderAttachDictionary for the
streaming state, and the adapters (needs a real MI355X).  Every stream is compared through dict_streams.check: result, error
code, decoded_size and every output byte; on success consumed, num_commands and num_metablocks too."""
import io
import os
import random
import sys

import pytest

import dict_streams as ds
import oracle_lib as oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
E = ds.E


def _workloads():
    sys.path.insert(0, ROOT)
    import workloads as w
    if not w.encoder_available():
        pytest.fail("libbrotlienc is not available: the GPU suite needs the encoder of the image for its synthetic streams (a skip here would let a third of the suite go green unrun)")
    return w


def _apply(cmds, dictionary):
    """what a command list puts out behind `dictionary`"""
    buf = bytearray(dictionary)
    for ins, clen, dist in cmds:
        buf += ins
        for _ in range(clen):
            buf.append(buf[-dist])
    return bytes(buf[len(dictionary):])


def _valid(comp, data, dictionary, flags=1):
    info, out = ds.expected(comp, len(data), flags, dictionary)
    assert (info.result, info.decoded_size) == (1, len(data)) and out == data, (info.result, info.error_code, info.decoded_size, len(data))
    return info


def _planned_shape(pkg, datas):
    """(BrotliAmdBatchLastGang, BrotliAmdBatchLastPool) that batch.h promises for a launch of these streams, with or without
    dictionaries: what the host plans for their compressed sizes on this device (BrotliAmdDebugPlanGangs)"""
    import ctypes
    import torch
    lib = pkg.load_library()
    lib.BrotliAmdDebugPlanGangs.restype = ctypes.c_uint32
    lib.BrotliAmdDebugPlanGangs.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    sizes = (ctypes.c_size_t * len(datas))(*[len(d) for d in datas])
    grid = ctypes.c_uint32(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kind = lib.BrotliAmdDebugPlanGangs(len(datas), cus, sizes, int(os.environ.get("BROTLI_AMD_GANG", -1)), int(os.environ.get("BROTLI_AMD_POOL", -1)), ctypes.byref(grid))
    return (1, 1) if kind == 0x108 else (max(1, kind), 0)


# ------------------------------------------------------------------ the streams (made once, shared by the tests)
_cache = {}


def _vector_set():
    """1. the reference's two vectors with test_gpu_engine._variants' set"""
    if "vec" not in _cache:
        rnd = random.Random(1)
        datas, caps, dicts = [], [], []
        for name, comp, d, exp in ds.vectors():
            _valid(comp, exp, d)
            a, b = ds.variants(rnd, comp, len(exp), damaged=10)
            for cut in (1, 2, len(comp) // 3, len(comp) - 1):   # truncated at several bytes
                a.append(comp[:cut]); b.append(len(exp) + 64)
            datas += a; caps += b; dicts += [d] * len(a)
        _cache["vec"] = (datas, caps, dicts)
    return _cache["vec"]


def _edge_stream(rnd, wbits, dsize, n):
    """a dictionary of dsize bytes and n bytes of data whose first command copies out of it, whatever its size"""
    maxb = (1 << wbits) - 16
    D = ds.text(rnd, dsize, "abcdefgh")
    first = [(b"", 5, min(dsize, maxb, 7))]
    head = _apply(first, D)
    rest = ds.related(rnd, D[-maxb:], n - len(head))
    cmds = first + E.greedy_commands(rest, max_dist=maxb, history=(D + head)[-maxb:])
    comp, data = ds.emit(cmds, wbits, D)
    assert data == head + rest
    _valid(comp, data, D)
    return comp, data, D


def _edge_set():
    """2. edges of the dictionary's size: valid, one byte short of output, truncated"""
    if "edge" not in _cache:
        rnd = random.Random(2)
        datas, caps, dicts = [], [], []
        for wbits, sizes in ((10, (1, 2, 15, 16, 17, 1007, 1008, 1009, 2500)), (16, (65519, 65520, 65521))):
            for dsize in sizes:
                for n in (300, 5000):
                    comp, data, D = _edge_stream(rnd, wbits, dsize, n)
                    datas += [comp, comp, comp[:len(comp) * 2 // 3]]; caps += [n, n - 1, n]; dicts += [D, D, D]
        _cache["edge"] = (datas, caps, dicts)
    return _cache["edge"]


def _boundary_set():
    """3. copies on the boundary between the dictionary and the output: hand-made command lists"""
    if "bound" not in _cache:
        rnd = random.Random(3)
        D = ds.text(rnd, 500, "ABCDEFGHIJKLMNOPQRSTUVWXYZ")
        tail = ds.text(rnd, 60, "xyz ")
        lists = []
        for lits in (b"", b"a", b"ab"):                                  # 0, 1, 2 literals, then a copy into the dictionary
            lists.append((16, D, [(lits, 10, 37 + len(lits)), (tail, 0, 0)]))
        for extra in (1, 2, 19):                                         # starts in the dictionary, runs into bytes it has just written
            lists.append((16, D, [(b"hello", 20, 5 + extra), (tail, 4, 9), (b"", 20, 5 + 20 + len(tail) + 4 + extra), (tail, 0, 0)]))
        lists.append((16, D, [(b"", 3000, 100), (tail, 0, 0)]))          # 3000 bytes that start 100 bytes in front of position 0
        lists.append((16, D, [(tail, 3000, len(tail) + 100), (tail, 0, 0)]))
        lists.append((16, D, [(tail, 3000, len(tail) + 100), (b"", 3000, 2900), (tail, 0, 0)]))
        lists.append((16, D, [(b"hello", 7, 5 + len(D)), (tail, 0, 0)]))  # exactly max_distance = P + the dictionary's size
        D10 = ds.text(rnd, 1008, "ABCDEFGH")
        lists.append((10, D10, [(b"hello", 7, 1008), (tail, 0, 0)]))     # ... = max_backward, the dictionary filling the window
        lists.append((10, D10[:400], [(tail, 30, len(tail) + 400), (tail, 0, 0)]))
        datas, caps, dicts = [], [], []
        for wbits, d, cmds in lists:
            comp, data = ds.emit(cmds, wbits, d)
            assert data == _apply(cmds, d) and ds.reaching(cmds, len(d)) >= 1
            _valid(comp, data, d)
            datas += [comp, comp, comp[:max(1, len(comp) - 3)]]; caps += [len(data), len(data) - 1, len(data)]; dicts += [d, d, d]
        # three windows' length at window 10: pos crosses max_backward - dict_size, then max_backward (one metablock, and several)
        D6 = ds.text(rnd, 600, "abcdefgh")
        for chunk in (None, 700):
            data = ds.related(rnd, D6, 3100)
            comp = ds.stream_for(data, 10, D6, chunk=chunk)
            _valid(comp, data, D6)
            a, b = ds.variants(rnd, comp, len(data), damaged=6)
            datas += a; caps += b; dicts += [D6] * len(a)
        _cache["bound"] = (datas, caps, dicts)
    return _cache["bound"]


# ------------------------------------------------------------------ 1 .. 5: one batch each
def test_reference_vectors(pkg):
    ds.check(pkg, *_vector_set(), flags=1, what="vectors")


def test_edges_of_the_dictionary_size(pkg):
    datas, caps, dicts = _edge_set()
    assert len(datas) == 72
    ds.check(pkg, datas, caps, dicts, flags=0, what="edges")


def test_copies_on_the_boundary(pkg):
    ds.check(pkg, *_boundary_set(), flags=0, what="boundary")


def test_first_literals_have_context_zero(pkg):
    """4. context-modelled plans over a dictionary that ends in b"Th" and one that ends in two zero bytes: a kernel that
    seeded the literal context from the dictionary would fail the first"""
    datas, caps, dicts = [], [], []
    for ending in (b"Th", b"\0\0"):
        rnd = random.Random(44)
        D = ds.text(rnd, 3000) + ending
        data = b"Zq" + ds.related(rnd, D, 5000)
        cmds = E.greedy_commands(data, max_dist=(1 << 16) - 16, history=D)
        assert len(cmds[0][0]) >= 2
        comp, out = ds.emit(cmds, 16, D, ds.context_plan(random.Random(5), cmds))
        _valid(comp, data, D)
        datas += [comp, comp]; caps += [len(data), len(data) - 1]; dicts += [D, D]
        comp2 = ds.stream_for(data, 16, D, plan="context", rnd=rnd, chunk=1500)
        _valid(comp2, data, D)
        datas.append(comp2); caps.append(len(data)); dicts.append(D)
    ds.check(pkg, datas, caps, dicts, flags=0, what="context")


def test_static_words_with_a_dictionary_attached(pkg):
    """5. a stream that was not made for the dictionary: the static dictionary's word numbers shift (distance - max_distance - 1)
    and some references become copies -- whatever the oracle says, errors included"""
    sys.path.insert(0, ROOT)
    import workloads as w
    comp, size, sha = w.fixture_streams("alice29.txt.compressed")[0]
    rnd = random.Random(5)
    datas, caps, dicts = [], [], []
    for dsize in (1, 1000, 70000):
        D = ds.text(rnd, dsize)
        for cap in (size, size + 1000, size // 2):
            datas.append(comp); caps.append(cap); dicts.append(D)
    datas.append(comp); caps.append(size); dicts.append(None)
    res = ds.check(pkg, datas, caps, dicts, flags=1, what="alice29 + dictionary")
    assert res[-1].result == 1 and res[-1].decoded_size == size


# ------------------------------------------------------------------ 6. engines
def test_engines_with_a_dictionary_attached(pkg):
    """The streams of test_gpu_engine.py::test_the_engine_takes_the_commands_of_the_streams_it_is_built_for with a 64 KiB dictionary
    attached, one batch of at most one stream a CU (sixteen-wave blocks; gangs of blocks, as without a dictionary): the oracle's
    bytes, and the command engines still take at least 90 % of their commands -- the bar that test sets without a dictionary.
    Among them one emitter stream of 256 KiB made FOR its dictionary (window 18, context-free): the oracle's bytes; what the
    engines take of it is printed, not judged (nobody has measured it)."""
    w = _workloads()
    streams = w.make_streams("long_backref", 6, 1 << 20, 1000)
    rnd = random.Random(6)
    D = ds.text(rnd, 65536)
    datas = [s[0] for s in streams]; caps = [s[1] for s in streams]; dicts = [D] * 6
    D2 = ds.text(rnd, 60000, "etaoinshrdlucmfwyp", 3000)
    data2 = ds.text(random.Random(66), 256 << 10, "etaoinshrdlucmfwyp", 3000)
    comp2 = ds.stream_for(data2, 18, D2)
    _valid(comp2, data2, D2)
    datas.append(comp2); caps.append(len(data2)); dicts.append(D2)
    batch = pkg.Batch(len(datas))
    try:
        res = ds.check(pkg, datas, caps, dicts, flags=1, what="engines", batch=batch)
        gang, pool = batch.last_gang(), batch.last_pool()
        # batch.h: a batch with dictionaries gets the launch shape of the same batch without them -- here gangs of blocks
        planned = _planned_shape(pkg, datas)
        assert planned[0] > 1, planned
        assert (gang, pool) == planned, (gang, pool, planned)
        plain, _ = batch.decode_host(datas, caps, 1)
        assert (batch.last_gang(), batch.last_pool()) == planned, (batch.last_gang(), batch.last_pool(), planned)
    finally:
        batch.close()
    for r in res[:6]:
        assert r.result == 1 and r.engine_commands >= 0.9 * r.num_commands, (r.engine_commands, r.num_commands)
    print("emitter stream against its dictionary: engine_commands %d of %d" % (res[6].engine_commands, res[6].num_commands))
    assert res[6].result == 1, (res[6].engine_commands, res[6].num_commands)


# ------------------------------------------------------------------ 7. launch shapes
def _mixed_set():
    """about forty streams of 1 .. 3, each with its own, a shared or no dictionary (the last: streams made for a dictionary
    decoded without it, and plain streams)"""
    if "mixed" not in _cache:
        rnd = random.Random(7)
        datas, caps, dicts = [], [], []
        for src in (_vector_set(), _edge_set(), _boundary_set()):
            idx = list(range(len(src[0])))
            rnd.shuffle(idx)
            for i in idx[:12]:
                datas.append(src[0][i]); caps.append(src[1][i]); dicts.append(src[2][i])
        for k in range(0, len(datas), 9):     # no dictionary for some
            dicts[k] = None
        shared = ds.text(rnd, 4000)
        for k in range(4):                     # one shared dictionary (the same object: one upload)
            data = ds.related(rnd, shared, 2000 + 300 * k)
            comp = ds.stream_for(data, 16, shared)
            datas.append(comp); caps.append(len(data)); dicts.append(shared)
        _cache["mixed"] = (datas, caps, dicts)
    return _cache["mixed"]


@pytest.mark.parametrize("n", [1, 3, 40])
def test_launch_shapes(pkg, n):
    datas, caps, dicts = _mixed_set()
    assert len(datas) == 40
    batch = pkg.Batch(n)
    try:
        ds.check(pkg, datas[:n], caps[:n], dicts[:n], flags=1, what="batch of %d" % n, batch=batch)
        shape = (batch.last_gang(), batch.last_pool())
        assert shape == _planned_shape(pkg, datas[:n]), (shape, _planned_shape(pkg, datas[:n]))
        # the same batch object without dictionaries (the existing entry point: its result exactly), then with them again
        ds.check(pkg, datas[:n], caps[:n], None, flags=1, what="batch of %d, no dictionaries" % n, batch=batch)
        assert shape == (batch.last_gang(), batch.last_pool())   # (batch.h: dictionaries do not change the launch's shape)
        ds.check(pkg, datas[:n], caps[:n], dicts[:n], flags=1, what="batch of %d, again" % n, batch=batch)
    finally:
        batch.close()


def test_six_hundred_streams(pkg):
    """the set repeated to 600 streams: small blocks, one-wave blocks, several streams a block one after the other"""
    datas, caps, dicts = _mixed_set()
    ds.check(pkg, datas * 15, caps * 15, dicts * 15, flags=1, what="600 streams")


# ------------------------------------------------------------------ 8. device pointers
def test_device_pointer_api_and_relaunch(pkg):
    import torch
    datas, caps, dicts = _mixed_set()
    n = len(datas)
    dev = torch.device("cuda:0")
    t_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev) for d in datas]
    t_out = [torch.zeros(max(1, c), dtype=torch.uint8, device=dev) for c in caps]
    held = {}
    for d in dicts:
        if d and id(d) not in held:
            held[id(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    dp = [held[id(d)].data_ptr() if d else None for d in dicts]
    dsz = [len(d) if d else 0 for d in dicts]
    batch = pkg.Batch(n)
    try:
        batch.decode_device([t.data_ptr() for t in t_in], [len(d) for d in datas], [t.data_ptr() for t in t_out], caps, 1, None, dict_ptrs=dp, dict_sizes=dsz)
        first = batch.wait()
        outs = [bytes(t_out[i][:min(first[i].decoded_size, caps[i])].cpu().numpy()) for i in range(n)]
        bad = ds.compare(first, outs, datas, caps, dicts, 1, "decode_device")
        assert not bad, (len(bad), bad[:8])
        for t in t_out:
            t.zero_()
        torch.cuda.synchronize()
        batch.relaunch()
        again = batch.wait()
        outs2 = [bytes(t_out[i][:min(again[i].decoded_size, caps[i])].cpu().numpy()) for i in range(n)]
        assert outs2 == outs
        assert [(r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands) for r in again] == [(r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands) for r in first]
    finally:
        batch.close()


# ------------------------------------------------------------------ 9. streaming
def _stream(pkg, comp, dictionary, in_chunk, out_chunk, max_calls=200000):
    st = pkg.DecoderState(large_window=True, dictionary=dictionary)
    out, pos, pending, calls, result = bytearray(), 0, b"", 0, None
    while True:
        if not pending and pos < len(comp):
            pending = comp[pos:pos + in_chunk]; pos += len(pending)
        elif not pending and result == pkg.RESULT_NEEDS_MORE_INPUT and not st.has_more_output():
            break   # the input has ended and everything decoded has been handed over
        result, used, got = st.decompress_stream(pending, out_chunk)
        pending = pending[used:]; out += got; calls += 1
        assert calls < max_calls
        if result in (pkg.RESULT_SUCCESS, pkg.RESULT_ERROR):
            break
    info = (result, st.error_code(), st.is_finished(), st.device_commands(), calls)
    st.close()
    return bytes(out), info


def _streaming_stream():
    if "streaming" not in _cache:
        rnd = random.Random(9)
        D = ds.text(rnd, 20000)
        data = ds.related(rnd, D, 150000)
        comp = ds.stream_for(data, 16, D, plan="context", rnd=rnd, chunk=40000)   # (more than two windows: the output is trimmed and re-based)
        _cache["streaming"] = (comp, data, D, _valid(comp, data, D))
    return _cache["streaming"]


@pytest.mark.parametrize("which,in_chunk,out_chunk", [("small", 1, 1), ("small", 1, 100), ("small", 1, 65536), ("small", 7, 1), ("small", 7, 100), ("large", 7, 65536),
                                                      ("small", 4096, 1), ("small", 4096, 100), ("large", 4096, 65536),
                                                      ("small", 1 << 30, 1), ("large", 1 << 30, 100), ("large", 1 << 30, 65536),
                                                      ("trimmed", 7, 65536), ("trimmed", 1 << 30, 100)])
def test_streaming_state_with_a_dictionary(pkg, which, in_chunk, out_chunk):
    """pieces of 1, 7 and 4096 bytes and the whole stream, each with output room of 1, 100 and 65536 bytes a call (a call with input
    is a launch: the one-byte pieces and the one-byte room go with a stream of a few thousand bytes); and small pieces over a
    stream of many windows, whose output the state trims and re-bases under the dictionary"""
    comp, data, D, info = _streaming_stream()
    if which != "large":
        if "streaming_" + which not in _cache:
            _cache["streaming_" + which] = _small_streaming_stream() if which == "small" else _trimmed_streaming_stream()
        comp, data, D = _cache["streaming_" + which]
        info = _valid(comp, data, D)
    out, (result, code, finished, commands, calls) = _stream(pkg, comp, D, in_chunk, out_chunk)
    assert (result, code, finished) == (1, 1, True) and out == data
    # test_gpu_streaming.py's bound for streams without a dictionary: a call is a launch from the last command boundary reached
    assert info.num_commands <= commands <= 2 * info.num_commands + 64 * calls, (commands, info.num_commands, calls)


def _small_streaming_stream():
    rnd = random.Random(91)
    D = ds.text(rnd, 3000)
    data = ds.related(rnd, D, 6000)   # (output room of one byte a call: a stream that takes thousands of calls, not hundreds of thousands)
    return ds.stream_for(data, 16, D, plan="context", rnd=rnd, chunk=2500), data, D


def _trimmed_streaming_stream():
    """window 10 and 200000 bytes of a short period: a few thousand compressed bytes, and an output that passes the state's 64 KiB
    and 128 KiB buffers -- it is trimmed to a window in front of the last command boundary and re-based (trim_buffers)"""
    rnd = random.Random(92)
    D = ds.text(rnd, 600)
    data = (ds.related(rnd, D, 400) * 500)[:200000]
    return ds.stream_for(data, 10, D, plan="context", rnd=rnd, chunk=50000), data, D


def test_streaming_truncated(pkg):
    comp, data, D, _ = _streaming_stream()
    cut = comp[:len(comp) * 3 // 5]
    info, exp = ds.oracle_decode_dict(cut, len(data), 1, D)
    assert info.result == 2
    out, (result, code, finished, _, _) = _stream(pkg, cut, D, 4096, 65536)
    assert (result, finished) == (2, False) and out == exp and len(out) == info.decoded_size
    # one dictionary per state, and none once it has decoded
    st = pkg.DecoderState(large_window=True, dictionary=D)
    assert not st.attach_dictionary(b"another")
    st.decompress_stream(comp[:10], 100)
    assert st.is_used() and not st.attach_dictionary(b"late")
    st.close()


def test_adapters_with_a_dictionary(pkg):
    comp, data, D, _ = _streaming_stream()
    assert pkg.Decompressor(io.BytesIO(comp), 4096, dictionary=D).read() == data
    sink = io.BytesIO()
    wtr = pkg.DecompressorWriter(sink, 4096, dictionary=D)
    for i in range(0, len(comp), 1000):
        wtr.write(comp[i:i + 1000])
    wtr.close()
    assert sink.getvalue() == data
    with pytest.raises(ValueError):
        pkg.Decompressor(io.BytesIO(comp[:len(comp) // 2]), 4096, dictionary=D).read()


def test_command_line_tool_with_a_dictionary(pkg, tmp_path):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools", "cli")])
    exe = os.path.join(ROOT, "tools", "cli", "brotli-decompressor")
    comp, data, D, _ = _streaming_stream()
    (tmp_path / "d.bin").write_bytes(D); (tmp_path / "in.br").write_bytes(comp)
    subprocess.check_call([exe, "-dict=" + str(tmp_path / "d.bin"), str(tmp_path / "in.br"), str(tmp_path / "out")], timeout=300)
    assert (tmp_path / "out").read_bytes() == data
