"""Stream sets (include/brotli/batch.h: BrotliAmdStreamSet) as far as they go without a GPU: the symbols, the life of a set,
the failures of a call as a whole, the states that end on the host, and -- on a box without a device -- that every state that
needed one ends as the solo call ends it."""
import ctypes
import os

import pytest

from conftest import ROOT, load_pkg

GOLD = os.path.join(ROOT, "tests", "golden", "testdata")
NEW = ["BrotliAmdStreamSetCreate", "BrotliAmdStreamSetDestroy", "BrotliAmdStreamSetDecompress", "BrotliAmdStreamSetLastLaunches",
       "BrotliAmdStreamSetLastTransfers", "BrotliAmdDebugRaggedCopy", "BrotliAmdDebugRaggedCopyTile"]


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


def test_symbols_are_declared_and_exported(lib):
    pkg = load_pkg()
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    for name in NEW:
        assert name in pkg.BATCH_H_SYMBOLS and hasattr(lib, name) and ("BROTLI_DEC_API" in header and name + "(" in header), name
    assert lib.BrotliAmdDebugRaggedCopyTile() >= 4096 and lib.BrotliAmdDebugRaggedCopyTile() % 16 == 0


def test_a_set_lives_and_dies_without_a_device(lib):
    for m in (0, 1, 64, 100000):
        h = lib.BrotliAmdStreamSetCreate(m)
        assert h
        assert lib.BrotliAmdStreamSetLastLaunches(h) == 0 and lib.BrotliAmdStreamSetLastTransfers(h) == 0
        lib.BrotliAmdStreamSetDestroy(h)
    lib.BrotliAmdStreamSetDestroy(None)
    assert lib.BrotliAmdStreamSetLastLaunches(None) == 0 and lib.BrotliAmdStreamSetLastTransfers(None) == 0
    pkg = load_pkg()
    s = pkg.StreamSet(4)
    assert s.decompress([], [], []) == [] and s.last_launches() == 0    # n == 0
    s.close()
    s.close()


class _Call:
    """the arrays of one raw BrotliAmdStreamSetDecompress call over n fresh states"""

    def __init__(self, lib, n, data=b"\x06", cap=16):
        self.lib, self.n = lib, n
        self.states = [lib.BrotliDecoderCreateInstance(None, None, None) for _ in range(n)]
        self.src = [ctypes.create_string_buffer(data, max(1, len(data))) for _ in range(n)]
        self.out = [ctypes.create_string_buffer(max(1, cap)) for _ in range(n)]
        self.st = (ctypes.c_void_p * n)(*self.states)
        self.ai = (ctypes.c_size_t * n)(*[len(data)] * n)
        self.ni = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in self.src])
        self.ao = (ctypes.c_size_t * n)(*[cap] * n)
        self.no = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in self.out])
        self.tot = (ctypes.c_size_t * n)()
        self.res = (ctypes.c_int * n)(*[-7] * n)

    def args(self):
        return [self.st, self.ai, self.ni, self.ao, self.no, self.tot, self.res]

    def untouched(self, data_len=1, cap=16):
        lib = self.lib
        return (all(lib.BrotliDecoderIsUsed(s) == 0 and lib.BrotliDecoderGetErrorCode(s) == 1 for s in self.states)
                and list(self.ai) == [data_len] * self.n and list(self.ao) == [cap] * self.n and list(self.res) == [-7] * self.n
                and list(self.ni) == [ctypes.addressof(b) for b in self.src] and list(self.no) == [ctypes.addressof(b) for b in self.out])

    def close(self):
        for s in self.states:
            self.lib.BrotliDecoderDestroyInstance(s)


def test_calls_that_fail_as_a_whole_touch_nothing(lib):
    dec = lib.BrotliAmdStreamSetDecompress
    h = lib.BrotliAmdStreamSetCreate(3)
    c = _Call(lib, 3)
    a = c.args()
    assert dec(None, 3, *a) < 0 and c.untouched()                          # no set
    for k in (0, 1, 2, 3, 4, 6):                                            # states, the four in/out arrays, results (total_out may be NULL)
        b = list(a); b[k] = None
        assert dec(h, 3, *b) < 0 and c.untouched(), k
    c.st[1] = None
    assert dec(h, 3, *a) < 0                                                # a NULL state
    c.st[1] = c.states[0]
    assert dec(h, 3, *a) < 0                                                # the same state twice
    c.st[1] = c.states[1]
    assert c.untouched()
    big = _Call(lib, 4)
    assert dec(h, 4, *big.args()) < 0 and big.untouched()                   # n > max_states
    assert dec(h, 0, *a) == 0 and c.untouched()                             # n == 0
    assert dec(h, 0, None, None, None, None, None, None, None) == 0
    assert lib.BrotliAmdStreamSetLastLaunches(h) == 0
    big.close(); c.close()
    lib.BrotliAmdStreamSetDestroy(h)


def test_states_without_input_end_on_the_host(lib):
    """no input: NEEDS_MORE_INPUT, nothing launched, nothing copied -- with or without a device; a latched error stays latched, and a
    call with bad slices latches INVALID_ARGUMENTS for its state alone"""
    pkg = load_pkg()
    s = pkg.StreamSet(8)
    states = [pkg.DecoderState(large_window=True) for _ in range(5)]
    assert s.decompress(states, [b""] * 5, [16] * 5) == [(2, 0, b"")] * 5
    assert (s.last_launches(), s.last_transfers()) == (0, 0)
    assert all(not st.is_used() and st.error_code() == 2 for st in states)
    # the solo function's argument check, per state: a NULL input pointer with a length
    L = pkg.load_library()
    c = _Call(L, 2, data=b"", cap=16)
    c.ai[0] = 5; c.ni[0] = None
    h = L.BrotliAmdStreamSetCreate(2)
    assert L.BrotliAmdStreamSetDecompress(h, 2, *c.args()) == 0
    assert list(c.res) == [0, 2] and L.BrotliDecoderGetErrorCode(c.states[0]) == -20 and L.BrotliDecoderGetErrorCode(c.states[1]) == 2
    # ... which is latched: the next call returns ERROR at once, whatever it is given
    c.ai[0] = 0
    assert L.BrotliAmdStreamSetDecompress(h, 2, *c.args()) == 0 and list(c.res) == [0, 2]
    assert L.BrotliAmdStreamSetLastLaunches(h) == 0 and L.BrotliAmdStreamSetLastTransfers(h) == 0
    L.BrotliAmdStreamSetDestroy(h)
    c.close()
    for st in states:
        st.close()
    s.close()


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour on a box without a GPU")
def test_without_a_device_every_state_ends_as_the_solo_call_ends_it():
    pkg = load_pkg()
    datas = [open(os.path.join(GOLD, n), "rb").read() for n in ("10x10y.compressed", "alice29.txt.compressed", "borked.compressed")] + [b""]
    solo = []
    for d in datas:
        st = pkg.DecoderState(large_window=True)
        solo.append((st.decompress_stream(d, 4096), st.error_code(), st.error_string(), st.is_used(), st.is_finished(), st.has_more_output()))
        st.close()
    assert solo[0][0] == (0, 0, b"") and solo[0][1] == -31 and "HIP" in solo[0][2]
    s = pkg.StreamSet(4)
    states = [pkg.DecoderState(large_window=True) for _ in datas]
    got = s.decompress(states, datas, [4096] * len(datas))
    assert [(g, st.error_code(), st.error_string(), st.is_used(), st.is_finished(), st.has_more_output()) for g, st in zip(got, states)] == solo
    assert (s.last_launches(), s.last_transfers()) == (0, 0)
    # the error is latched in the states that needed the device; the one without input goes on as before
    assert s.decompress(states, datas, [4096] * len(datas)) == [(0, 0, b"")] * 3 + [(2, 0, b"")]
    # ... and a state may go from the set to solo calls and back: the same answers
    assert states[0].decompress_stream(datas[0], 16) == (0, 0, b"") and states[3].decompress_stream(b"", 16) == (2, 0, b"")
    for st in states:
        st.close()
    s.close()
