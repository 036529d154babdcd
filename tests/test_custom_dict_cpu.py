"""Custom (LZ77 prefix) dictionaries without a GPU: the emitter's `dictionary=` against the CPU oracle, the library's new entry
points (include/brotli/batch.h), BrotliAmdDecoderAttachDictionary's answers on an instance that never decodes, and the loud
failures where no HIP device is usable."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

import dict_streams as ds
import oracle_lib as oracle
from conftest import ROOT, load_pkg

E = ds.E


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    return pkg.load_library()


def _roundtrip(comp, data, dictionary, flags=0):
    info, out = ds.oracle_decode_dict(comp, len(data), flags, dictionary)
    assert (info.result, info.decoded_size, info.consumed) == (1, len(data), len(comp))
    assert out == data


@pytest.mark.parametrize("wbits,dsize", [(10, 1008), (16, 20000), (18, 65520), (22, 30000)])
def test_emitter_streams_for_a_dictionary_decode_to_their_data(wbits, dsize):
    """context-free plans: copies reach into the dictionary, and without it the stream is another stream"""
    rnd = random.Random(wbits * 1000 + dsize)
    D = ds.text(rnd, dsize)
    data = ds.related(rnd, D, 6000)
    cmds = E.greedy_commands(data, max_dist=(1 << wbits) - 16, history=D[-((1 << wbits) - 16):])
    assert ds.reaching(cmds, len(D)) >= 10
    comp, out = ds.emit(cmds, wbits, D)
    assert out == data
    _roundtrip(comp, data, D)
    info, got = oracle.decode(comp, len(data), 0)
    assert info.result != 1 or got != data


@pytest.mark.parametrize("ending", [b"Th", b"9 ", b"\0\0"])
def test_context_modelled_plan_over_a_dictionary_that_ends_in_anything(ending):
    """modes 0 to 3 with a chosen map: the first two literals have context (0, 0) whatever the dictionary's last bytes are
    (decode.rs:2466-2476) -- `prev=D`, the way round before `dictionary=` existed, is only right for a dictionary that ends in two zero bytes"""
    rnd = random.Random(77)
    D = ds.text(rnd, 3000) + ending
    data = b"Zq" + ds.related(rnd, D, 5000)   # (two literals first: the ones whose context is at stake)
    cmds = E.greedy_commands(data, max_dist=(1 << 16) - 16, history=D)
    assert len(cmds[0][0]) >= 2 and ds.reaching(cmds, len(D)) >= 10
    plan = ds.context_plan(random.Random(5), cmds)
    comp, out = ds.emit(cmds, 16, D, plan)
    assert out == data
    _roundtrip(comp, data, D)
    # the old way round models those two literals with the dictionary's last bytes: the same stream only where they are zero
    w = E.BitWriter(); E.write_stream_header(w, 16)
    E.emit_compressed(w, cmds, plan, True, prev=D)
    assert (w.finish() == comp) == (ending == b"\0\0")


def test_several_metablocks_and_a_dictionary_longer_than_the_window():
    rnd = random.Random(9)
    D = ds.text(rnd, 2500)
    data = ds.related(rnd, D[-1008:], 3200)
    comp = ds.stream_for(data, 10, D, plan="context", rnd=rnd, chunk=700)
    _roundtrip(comp, data, D)


def test_the_default_leaves_the_emitter_as_it_was():
    """tests/golden/emitter/ is pinned by hashes (test_oracle.py::test_emitter_is_deterministic): one vector again, with the argument spelled out"""
    rnd = random.Random(3)
    data = ds.text(rnd, 4000)
    cmds = E.greedy_commands(data)
    a, b = E.BitWriter(), E.BitWriter()
    for w in (a, b):
        E.write_stream_header(w, 18)
    E.emit_compressed(a, cmds, E.Plan(), True)
    E.emit_compressed(b, cmds, E.Plan(), True, dictionary=b"")
    assert a.finish() == b.finish()


def test_reference_vectors_still_decode():
    for name, comp, d, exp in ds.vectors():
        info, out = ds.oracle_decode_dict(comp, len(exp) + 64, 1, d)
        assert (info.result, info.decoded_size) == (1, len(exp)) and out == exp, name


def test_library_exports_the_dictionary_entry_points(lib):
    pkg = load_pkg()
    for name in ("BrotliAmdBatchDecodeDeviceDict", "BrotliAmdBatchDecodeHostDict", "BrotliAmdDecoderAttachDictionary"):
        assert name in pkg.BATCH_H_SYMBOLS and hasattr(lib, name), name


def test_attach_dictionary_answers(lib):
    """TRUE on a fresh instance and for size 0; FALSE for NULL data with a size, for a second dictionary, for no instance"""
    attach = lib.BrotliAmdDecoderAttachDictionary   # (argument types: the binding's, void pointers -- which take bytes)
    st = lib.BrotliDecoderCreateInstance(None, None, None)
    assert attach(st, None, 0) == 1 and attach(st, b"x", 0) == 1     # no-ops
    assert attach(st, None, 5) == 0
    assert attach(st, b"hello dictionary", 16) == 1
    assert attach(st, b"x", 0) == 1                                   # still a no-op
    assert attach(st, b"another", 7) == 0                             # one dictionary per instance
    assert lib.BrotliDecoderIsUsed(st) == 0
    lib.BrotliDecoderDestroyInstance(st)
    assert attach(None, b"abc", 3) == 0
    # through the allocator callbacks the instance was made with: the copy is the instance's
    alloc_t = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
    free_t = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p; libc.malloc.argtypes = [ctypes.c_size_t]; libc.free.argtypes = [ctypes.c_void_p]
    live = set()

    def _alloc(opaque, n):
        p = libc.malloc(n); live.add(p); return p

    def _free(opaque, p):
        if p:
            live.discard(p); libc.free(p)
    a, f = alloc_t(_alloc), free_t(_free)
    st = lib.BrotliDecoderCreateInstance(ctypes.cast(a, ctypes.c_void_p), ctypes.cast(f, ctypes.c_void_p), None)
    buf = ctypes.create_string_buffer(b"q" * 5000)
    assert attach(st, buf, 5000) == 1 and len(live) == 2
    ctypes.memset(buf, 0, 5000)   # (the caller's buffer may go: the bytes were copied)
    lib.BrotliDecoderDestroyInstance(st)
    assert not live


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour on a box without a GPU")
def test_dictionary_entry_points_fail_loudly_without_a_device(lib):
    pkg = load_pkg()
    with pytest.raises(RuntimeError):
        pkg.Batch(2)
    # (no batch object can exist: the entry points refuse a NULL one)
    lib.BrotliAmdBatchDecodeHostDict.restype = ctypes.c_int
    lib.BrotliAmdBatchDecodeDeviceDict.restype = ctypes.c_int
    assert lib.BrotliAmdBatchDecodeHostDict(None, 1, None, None, None, None, None, None, 0, None) < 0
    assert lib.BrotliAmdBatchDecodeDeviceDict(None, 1, None, None, None, None, None, None, 0, None) < 0
    assert "invalid batch arguments" in pkg.last_error()
    # a streaming instance takes its dictionary and fails at the first decode, with the runtime's message
    name, comp, d, exp = ds.vectors()[0]
    st = pkg.DecoderState(large_window=True, dictionary=d)
    r, used, out = st.decompress_stream(comp, 4096)
    assert (r, out) == (0, b"") and st.error_code() == -31 and "HIP" in st.error_string()
    st.close()


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour on a box without a GPU")
def test_command_line_tool_takes_a_dictionary(lib, tmp_path):
    """-dict=FILE is read and handed on: without a device the tool ends with the runtime's message, not with 'not supported'"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools", "cli")])
    exe = os.path.join(ROOT, "tools", "cli", "brotli-decompressor")
    name, comp, d, exp = ds.vectors()[0]
    (tmp_path / "d.bin").write_bytes(d); (tmp_path / "in.br").write_bytes(comp)
    p = subprocess.run([exe, "-dict=" + str(tmp_path / "d.bin"), str(tmp_path / "in.br"), str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"HIP" in p.stderr and b"not supported" not in p.stderr, p.stderr
    p = subprocess.run([exe, "-dict=" + str(tmp_path / "missing.bin"), str(tmp_path / "in.br")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"missing.bin" in p.stderr
