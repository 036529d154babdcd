"""Batches whose decoded sizes nobody knows (needs a real MI355X): the size-walk kernel (csrc/brotli_size_kernels.hip) against the host's
walk, field for field, and the packed decode (BrotliAmdBatchDecodeDevicePacked / HostPacked) against the CPU oracle -- result, error
code, decoded_size, the offsets and EVERY byte of the packed buffer: the streams lie back to back in it without padding, so a store
wider than a stream's slot would land in its neighbour."""
import ctypes
import random
import sys

import pytest

import dict_streams as ds
import oracle_lib as oracle
import size_streams as ss
from conftest import ROOT

pytestmark = pytest.mark.gpu
FLAGS = 1   # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64  # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT

_cache = {}


def _upload(datas, align=lambda k: 0):
    """the streams in ONE device arena, stream k at an address of alignment align(k) mod 16 -> (tensor, pointers)"""
    import numpy as np
    import torch
    offs, at = [], 0
    for k, d in enumerate(datas):
        at = (at + 15) // 16 * 16 + align(k)
        offs.append(at); at += len(d)
    host = np.zeros(at + 16, dtype=np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, [t.data_ptr() + o for o in offs]


def _true_size(data):
    """the decoded size of a stream that decodes, else room enough for whatever it delivers before it fails"""
    if bytes(data) not in _cache:
        cap = 1 << 20
        info, _ = oracle.decode(data, cap, FLAGS)
        while info.result == oracle.RESULT_NEEDS_MORE_OUTPUT:
            cap *= 4
            info, _ = oracle.decode(data, cap, FLAGS)
        _cache[bytes(data)] = info.decoded_size if info.result == oracle.RESULT_SUCCESS else cap
    return _cache[bytes(data)]


def _check_packed(results, blob, offsets, datas, dicts=None, caps=None, what=""):
    """every stream's triple, the offsets and the whole packed buffer against the oracle's decode into caps[i] bytes (None: the true size)"""
    exp_blob, exp_offsets, bad = bytearray(), [0], []
    for i, d in enumerate(datas):
        cap = caps[i] if caps else _true_size(d)
        info, exp = ds.expected(d, cap, FLAGS, dicts[i] if dicts else None)
        r = results[i]
        if (r.result, r.error_code, r.decoded_size) != (info.result, info.error_code, info.decoded_size):
            bad.append((i, what, (r.result, r.error_code, r.decoded_size), (info.result, info.error_code, info.decoded_size), len(d), cap))
        exp_blob += exp; exp_offsets.append(len(exp_blob))
    assert not bad, (len(bad), bad[:8])
    assert offsets == exp_offsets, what
    assert len(blob) == len(exp_blob), what
    if blob != bytes(exp_blob):
        at = next(k for k in range(len(blob)) if blob[k] != exp_blob[k])
        raise AssertionError((what, "first wrong byte", at, "of stream", next(i for i in range(len(datas)) if exp_offsets[i + 1] > at)))


def _packed_host(pkg, datas, dicts=None, max_out=0, batch=None):
    """decode_device_packed over an arena of the streams, and a fetch -> (results, blob, offsets, launches, copies)"""
    import torch
    b = batch or pkg.Batch(max(1, len(datas)))
    try:
        t, ptrs = _upload(datas, lambda k: (5 * k) % 16)
        dp = dsz = None
        held = {}
        if dicts:
            for d in dicts:
                if d and id(d) not in held:
                    held[id(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
            torch.cuda.synchronize()
            dp = [held[id(d)].data_ptr() if d else None for d in dicts]
            dsz = [len(d) if d else 0 for d in dicts]
        results, ptr, offsets = b.decode_device_packed(ptrs, [len(d) for d in datas], dp, dsz, max_out, FLAGS)
        assert len(offsets) == len(datas) + 1 and (ptr != 0 or offsets[-1] == 0)
        blob = b.packed_fetch(offsets[-1])
        return results, blob, offsets, b.last_packed_launches(), b.last_packed_copies()
    finally:
        if batch is None:
            b.close()


# ------------------------------------------------------------------ 1. the kernel against the host's walk
def _walk_set():
    if "walk" not in _cache:
        datas = [d for which in ("testdata", "emitter", "param_corpus") for _, d, _ in ss.corpus(which)]
        datas.append(ss.long_walk_stream()[0])
        first_prefix = len(datas)
        for name in ss.SHORT_GOLDEN:
            s = ss.golden(name)
            assert len(s) < 100
            datas += [s[:n] for n in range(len(s) + 1)]
        _cache["walk"] = (datas, first_prefix)
    return _cache["walk"]


def test_size_walk_kernel_equals_the_host_function(pkg):
    datas, first_prefix = _walk_set()
    # the corpus at every alignment in turn; prefix n of a stream at alignment n mod 16, each right behind its neighbour's sixteen
    t, ptrs = _upload(datas, lambda k: k % 16 if k < first_prefix else (k - first_prefix) % 16)
    assert {p % 16 for p in ptrs[first_prefix:]} == set(range(16))
    b = pkg.Batch(1)   # (the walk is not bound by max_streams)
    try:
        for flags in (FLAGS, 0):
            hints = b.size_hints(ptrs, [len(d) for d in datas], flags)
            bad = [(i, len(datas[i]), hints[i].astuple(), pkg.size_walk(datas[i], flags).astuple()) for i in range(len(datas))
                   if hints[i].astuple() != pkg.size_walk(datas[i], flags).astuple()]
            assert not bad, (flags, len(bad), bad[:8])
    finally:
        b.close()


def test_size_walk_kernel_launch_edges(pkg):
    """0, 1, 63, 64, 65 and 1000 copies of one stream: wave and block edges; and one more than a whole grid's lanes: the grid-stride tail"""
    import torch
    stream = ss.long_walk_stream()[0]
    want = pkg.size_walk(stream).astuple()
    t, (p,) = _upload([stream], lambda k: 3)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = pkg.Batch(1)
    try:
        for n in (0, 1, 63, 64, 65, 1000, cus * 4 * 256 + 77):
            hints = b.size_hints([p] * n, [len(stream)] * n)
            assert len(hints) == n
            wrong = [i for i in range(n) if hints[i].astuple() != want]
            assert not wrong, (n, len(wrong), wrong[:8])
    finally:
        b.close()


# ------------------------------------------------------------------ 2. the golden batch
def _golden_set():
    datas = [d for n, d, size in ss.corpus("testdata") if n != "rnd_chunk.br"]
    datas.append(ss.golden("alice29.txt.compressed")[:20000])   # (truncated)
    return datas


def test_packed_golden_batch(pkg):
    datas = _golden_set()
    names = [n for n, _, _ in ss.corpus("testdata")]
    assert "borked.compressed" in names and len(datas) >= 54
    results, blob, offsets, launches, copies = _packed_host(pkg, datas)
    _check_packed(results, blob, offsets, datas, what="golden")
    assert sum(1 for r in results if r.result == 1) >= 52
    assert launches >= 1 and copies >= 1   # (streams that failed do not fill their slots: a gather)


def test_packed_rnd_chunk_grows_round_after_round(pkg):
    """rnd_chunk.br: 1151 compressed bytes that decode to 100 011 280 -- six times the first guess of some 16 MiB, so several growth rounds on
    large data, beside a small document that must come through untouched in front of it"""
    import hashlib
    stream = ss.golden("rnd_chunk.br")
    size = next(s for n, _, s in ss.corpus("testdata") if n == "rnd_chunk.br")
    info, exp = oracle.decode(stream, size, FLAGS)
    assert (info.result, info.decoded_size) == (1, size) and size == 100011280
    h = pkg.size_walk(stream)
    assert h.exact == 0 and h.bytes + 6 * len(stream) < size // 4
    doc, raw = _documents()[0]
    b = pkg.Batch(2)
    try:
        t, ptrs = _upload([doc, stream], lambda k: 7 * k + 1)
        results, ptr, offsets = b.decode_device_packed(ptrs, [len(doc), len(stream)], None, None, 0, FLAGS)
        launches, copies = b.last_packed_launches(), b.last_packed_copies()
        blob = b.packed_fetch(offsets[-1])
    finally:
        b.close()
    print("rnd_chunk.br: %d decode launches, %d ragged copies" % (launches, copies))
    assert [(r.result, r.error_code, r.decoded_size) for r in results] == [(1, 1, len(raw)), (info.result, info.error_code, size)]
    assert offsets == [0, len(raw), len(raw) + size]
    assert launches >= 3 and copies == launches   # (a copy a growth round, and the gather)
    assert blob[:len(raw)] == raw
    assert hashlib.sha256(blob[len(raw):]).digest() == hashlib.sha256(exp).digest()


# ------------------------------------------------------------------ 3. exact hints: one launch, no copy
def _documents(n_distinct=30):
    if "docs" not in _cache:
        rnd = random.Random(300)
        docs = []
        for k in range(n_distinct):
            data = ds.text(rnd, rnd.randrange(1, 6000), "etaoinshrdlucmfwyp", 300)
            docs.append((ds.stream_for(data, rnd.choice([10, 16, 18, 22]), None), data))
        _cache["docs"] = docs
    return _cache["docs"]


def test_packed_exact_hints_need_one_launch_and_no_copy(pkg):
    docs = _documents()
    rnd = random.Random(301)
    picks = [docs[k % len(docs)] if k < len(docs) else rnd.choice(docs) for k in range(300)]
    datas = [c for c, _ in picks]
    assert all(pkg.size_walk(c).astuple()[2:] == (1, 0) and pkg.size_walk(c).bytes == len(d) for c, d in docs)
    results, blob, offsets, launches, copies = _packed_host(pkg, datas)
    assert (launches, copies) == (1, 0), (launches, copies)
    assert all(r.result == 1 for r in results)
    assert blob == b"".join(d for _, d in picks)
    _check_packed(results, blob, offsets, datas, what="documents")


# ------------------------------------------------------------------ 4. growth, 5. the limit
def _growth_set():
    grow, raw = ss.growing_stream()
    assert len(grow) < 2000 and len(raw) > 3 * (200 << 10)
    info, out = oracle.decode(grow, len(raw), FLAGS)
    assert info.result == 1 and out == raw
    h = pkg_walk(grow)
    assert h.exact == 0 and h.bytes < 65536 * 4   # (the first metablock alone is known: the first capacity is far from the whole)
    docs = [c for c, _ in _documents()[:6]]
    return docs[:3] + [ss.golden("reducetostream.map.compressed"), grow] + docs[3:] + [ss.golden("alice29.txt.compressed"), ss.golden("borked.compressed")]


def pkg_walk(data):
    from conftest import load_pkg
    return load_pkg().size_walk(data)


def test_packed_growth(pkg):
    datas = _growth_set()
    results, blob, offsets, launches, copies = _packed_host(pkg, datas)
    assert launches >= 2 and copies >= 2, (launches, copies)   # (a copy a growth round, and the gather)
    _check_packed(results, blob, offsets, datas, what="growth")
    assert results[3].result == 1 and results[3].decoded_size == 950881 and results[4].result == 1


def test_packed_output_limit(pkg):
    """max_out_bytes = 100000 against BrotliAmdBatchDecodeDevice with out_caps = 100000 and the eager flag: the same results, the same bytes"""
    import torch
    datas = _growth_set()
    n, limit = len(datas), 100000
    results, blob, offsets, launches, copies = _packed_host(pkg, datas, max_out=limit)
    t, ptrs = _upload(datas)
    outs = [torch.zeros(limit, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()
    b = pkg.Batch(n)
    try:
        b.decode_device(ptrs, [len(d) for d in datas], [o.data_ptr() for o in outs], [limit] * n, FLAGS | EAGER)
        plain = b.wait()
    finally:
        b.close()
    key = lambda r: (r.result, r.error_code, r.decoded_size, r.consumed, r.produced)
    assert [key(r) for r in results] == [key(r) for r in plain]
    assert any(r.result == 3 and r.decoded_size == limit for r in results) and any(r.result == 1 for r in results)
    assert offsets == [sum(r.decoded_size for r in plain[:i]) for i in range(n + 1)]
    for i in range(n):
        assert blob[offsets[i]:offsets[i + 1]] == bytes(outs[i][:plain[i].decoded_size].cpu().numpy()), i


# ------------------------------------------------------------------ 6. dictionaries
def test_packed_with_custom_dictionaries(pkg):
    rnd = random.Random(600)
    shared = ds.text(rnd, 4000)
    datas, dicts = [], []
    for k in range(12):
        data = ds.related(rnd, shared, 500 + 700 * k)
        datas.append(ds.stream_for(data, 16, shared, chunk=None if k % 3 else 1500)); dicts.append(shared)   # (several metablocks: estimates and growth)
    own = ds.text(rnd, 900, "ABCDEFGH")
    data = ds.related(rnd, own, 3000)
    datas.append(ds.stream_for(data, 10, own)); dicts.append(own)
    for c, _ in _documents()[:5]:   # ... and streams without one
        datas.append(c); dicts.append(None)
    order = list(range(len(datas)))
    rnd.shuffle(order)
    datas = [datas[i] for i in order]; dicts = [dicts[i] for i in order]
    caps = []
    for d, dic in zip(datas, dicts):
        info, _ = ds.expected(d, 1 << 20, FLAGS, dic)
        assert info.result == 1
        caps.append(info.decoded_size)
    results, blob, offsets, launches, copies = _packed_host(pkg, datas, dicts=dicts)
    _check_packed(results, blob, offsets, datas, dicts=dicts, caps=caps, what="dictionaries")
    # the host form: each distinct dictionary uploaded once, the same bytes
    b = pkg.Batch(len(datas))
    try:
        res2, outs2 = b.decode_packed(datas, dicts=dicts)
    finally:
        b.close()
    assert b"".join(outs2) == blob and [r.decoded_size for r in res2] == [r.decoded_size for r in results]


# ------------------------------------------------------------------ 7. gangs
def test_packed_gang_shape(pkg):
    sys.path.insert(0, ROOT)
    import workloads as w
    if not w.encoder_available():
        pytest.fail("libbrotlienc is not available: the GPU suite needs the encoder of the image for its synthetic streams")
    raws = [w.high_entropy_stream(7700 + k, (1 << 20) + 4097 * k) for k in range(2)]
    datas = [w.brotli_compress(r, 5, 22) for r in raws]
    assert all(len(d) >= 256 << 10 for d in datas)
    for d, r in zip(datas, raws):
        _cache[bytes(d)] = len(r)
    b = pkg.Batch(2)
    try:
        results, blob, offsets, launches, copies = _packed_host(pkg, datas, batch=b)
        assert b._L.BrotliAmdBatchLastGang(b._h) > 1
    finally:
        b.close()
    assert blob == b"".join(raws)
    _check_packed(results, blob, offsets, datas, what="gangs")


# ------------------------------------------------------------------ 8. one batch object, call after call
def test_packed_reuse_of_a_batch_object(pkg):
    import torch
    datas = _growth_set()
    docs = _documents()
    b = pkg.Batch(64)
    try:
        results, blob, offsets, _, _ = _packed_host(pkg, datas, batch=b)
        _check_packed(results, blob, offsets, datas, what="first packed call")
        ms_packed = b.last_kernel_ms()   # (all decode launches of the packed call)
        assert ms_packed > 0 and b.last_packed_launches() >= 2
        # a plain decode_device + wait with known capacities and the default (not eager) flags in between: it ends the packed result ...
        plain = [c for c, _ in docs[:7]] + [ss.golden("borked.compressed"), docs[7][0]]
        caps = [len(d) for _, d in docs[:7]] + [4096, len(docs[7][1]) - 1]   # (one fails, one is a byte short: the reference's verdict, not the eager one)
        t, ptrs = _upload(plain, lambda k: 3 * k)
        t_out = [torch.zeros(max(1, c), dtype=torch.uint8, device="cuda:0") for c in caps]
        torch.cuda.synchronize()
        b.decode_device(ptrs, [len(d) for d in plain], [o.data_ptr() for o in t_out], caps, FLAGS)
        res = b.wait()
        outs = [bytes(t_out[i][:min(res[i].decoded_size, caps[i])].cpu().numpy()) for i in range(len(plain))]
        bad = ds.compare(res, outs, plain, caps, None, FLAGS, "decode_device between packed calls")
        assert not bad, bad
        assert res[-1].result == 3 and res[-2].result == 0
        assert 0 < b.last_kernel_ms() != ms_packed   # (this launch's, not the packed call's)
        offs = ctypes.POINTER(ctypes.c_uint64)()
        assert not b._L.BrotliAmdBatchPackedOutput(b._h, ctypes.byref(offs)) and not offs
        assert (b.last_packed_launches(), b.last_packed_copies()) == (0, 0)
        with pytest.raises(RuntimeError):
            b.packed_fetch(1)
        b.relaunch(); again = b.wait()   # ... and is itself what Relaunch comes back to
        assert [(r.result, r.error_code, r.decoded_size) for r in again] == [(r.result, r.error_code, r.decoded_size) for r in res]
        # ... and the host form of a plain decode
        res, outs = b.decode_host(plain[:7], caps[:7], FLAGS)
        assert all(r.result == 1 for r in res) and outs == [d for _, d in docs[:7]]
        # another n; and the host form gives the same bytes as the device form and a fetch
        second = [c for c, _ in docs[:40]] + datas[3:5]
        results, blob, offsets, launches, copies = _packed_host(pkg, second, batch=b)
        _check_packed(results, blob, offsets, second, what="second packed call")
        res2, outs2 = b.decode_packed(second)
        assert b"".join(outs2) == blob and [len(o) for o in outs2] == [offsets[i + 1] - offsets[i] for i in range(len(second))]
        assert [(r.result, r.error_code, r.decoded_size) for r in res2] == [(r.result, r.error_code, r.decoded_size) for r in results]
        assert (b.last_packed_launches(), b.last_packed_copies()) == (launches, copies)
        # n == 0
        results, ptr, offsets = b.decode_device_packed([], [])
        assert results == [] and offsets == [0] and b.last_packed_launches() == 0
    finally:
        b.close()
    torch.cuda.synchronize()
