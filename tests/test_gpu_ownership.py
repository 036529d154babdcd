"""Nothing leaks (needs a real MI355X): every device and pinned allocation of the host side goes through one owning buffer type
(csrc/brotli_host.h: Buffer) that counts its live bytes, and brotli_amd_debug_live_bytes reports the counts.  The smallest shapes that
reach every buffer -- a batch object's staging arenas, pinned sides, dictionary arena, settle scratch, size-walk buffer, packed slots, grown
rounds and tight output, a streaming state's input, output (re-based) and dictionary, a stream set's segment tables and staging -- are used,
the objects destroyed, and both counts must be back where they were."""
import ctypes

import pytest

import dict_streams as ds
import oracle_lib as oracle
import size_streams as ss

pytestmark = pytest.mark.gpu
FLAGS = 1   # BROTLI_AMD_BATCH_LARGE_WINDOW


def _live(L):
    dev, pin = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L.brotli_amd_debug_live_bytes.restype = None
    L.brotli_amd_debug_live_bytes.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.brotli_amd_debug_live_bytes(ctypes.byref(dev), ctypes.byref(pin))
    return dev.value, pin.value


def _state_bytes(L, st):
    L.brotli_amd_debug_stream_device_bytes.restype = ctypes.c_size_t
    L.brotli_amd_debug_stream_device_bytes.argtypes = [ctypes.c_void_p]
    return int(L.brotli_amd_debug_stream_device_bytes(st._h))


def test_every_buffer_goes_with_its_owner(pkg):
    import torch
    L = pkg.load_library()
    fox, ukk, x10 = (ss.golden(n) for n in ("quickfox.compressed", "ukkonooa.compressed", "10x10y.compressed"))
    sizes = {bytes(d): oracle.decode(d, 1 << 16, FLAGS)[0].decoded_size for d in (fox, ukk, x10)}
    _, v_comp, v_dict, v_exp = ds.vectors()[0]
    grow, grow_raw = ss.growing_stream()

    # 1. the per-device dictionary exists (it stays for the life of the process and is not counted); the baseline
    b = pkg.Batch(1)
    res, outs = b.decode_host([fox], [sizes[bytes(fox)]], FLAGS)
    assert res[0].result == 1
    b.close()
    base = _live(L)

    # 2. a batch object through every entry point that owns memory, three times over
    for _ in range(3):
        b = pkg.Batch(4)
        # host buffers, one custom dictionary shared by two streams: the three staging arenas and the pinned sides
        datas, dicts = [v_comp, v_comp, fox, ukk], [v_dict, v_dict, None, None]
        caps = [len(v_exp), len(v_exp), sizes[bytes(fox)], sizes[bytes(ukk)]]
        res, outs = b.decode_host(datas, caps, FLAGS, dicts=dicts)
        assert [r.result for r in res] == [1] * 4 and outs[0] == outs[1] == v_exp
        # device buffers, one output too small: the settle pass and its scratch
        datas = [fox, ukk, x10, fox]
        caps = [sizes[bytes(d)] for d in datas]
        caps[1] = 50
        d_in = [torch.frombuffer(bytearray(d) + bytearray(256), dtype=torch.uint8).cuda() for d in datas]
        d_out = [torch.zeros(c + 256, dtype=torch.uint8, device="cuda") for c in caps]
        before = _live(L)[0]
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [t.data_ptr() for t in d_out], caps, FLAGS)
        res = b.wait()
        for r, d, c in zip(res, datas, caps):
            info, _ = oracle.decode(d, c, FLAGS)
            assert (r.result, r.error_code, r.decoded_size) == (info.result, info.error_code, info.decoded_size)
        assert res[1].result != 1 and _live(L)[0] > before   # (the stream with the short buffer was looked at again: scratch up to its flush point)
        # size hints: the size walk's buffer
        hints = b.size_hints([t.data_ptr() for t in d_in], [len(d) for d in datas], FLAGS)
        assert [h.astuple() for h in hints] == [pkg.size_walk(d, FLAGS).astuple() for d in datas]
        # a packed decode in which one stream's hint is not exact: slots, a grown round, the gather into the tight buffer
        datas = [fox, grow, ukk, x10]
        res, outs = b.decode_packed(datas, flags=FLAGS)
        assert b.last_packed_launches() >= 2 and b.last_packed_copies() >= 2
        assert [r.result for r in res] == [1] * 4 and outs[1] == grow_raw and len(outs[0]) == sizes[bytes(fox)]
        assert _live(L)[0] > base[0] and _live(L)[1] > base[1]
        b.close()
        del d_in, d_out
        assert _live(L) == base

    # 3. a streaming state with a dictionary, two chunks, its device output buffer re-based (it starts at 64 KiB; the stream decodes to 600 KiB)
    st = pkg.DecoderState(large_window=True, dictionary=v_dict)
    half = len(grow) // 2
    got = b""
    for chunk in (grow[:half], grow[half:]):
        r, used, out = st.decompress_stream(chunk, 1 << 20)
        assert used == len(chunk)
        got += out
    assert r == 1 and got == grow_raw
    held = _state_bytes(L, st)
    assert held > len(grow_raw)   # (the output buffer has grown)
    # 6. with the object alive, the count covers what it reports
    assert _live(L)[0] - base[0] >= held + len(v_dict)

    # 4. a stream set of three states through one call
    states = [pkg.DecoderState(large_window=True) for _ in range(3)]
    sset = pkg.StreamSet(3)
    outs = sset.decompress(states, [fox, ukk, x10], [1 << 16] * 3)
    assert [o[0] for o in outs] == [1, 1, 1] and sset.last_launches() == 1
    assert [len(o[2]) for o in outs] == [sizes[bytes(d)] for d in (fox, ukk, x10)]
    assert _live(L)[0] - base[0] >= held + sum(_state_bytes(L, s) for s in states)
    sset.close()
    for s in states + [st]:
        s.close()

    # 5. both counts are back at the baseline, exactly
    assert _live(L) == base
