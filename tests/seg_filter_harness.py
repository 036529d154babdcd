"""What the GPU tests of the element filters (test_gpu_unshuffle.py, test_gpu_undelta.py, test_gpu_bitunshuffle.py, test_gpu_bitunpack.py,
test_gpu_unvarint.py, test_gpu_unrle.py, test_gpu_undbp.py) share: sources from one seeded read-only buffer, destinations from one buffer prefilled
with a sentinel pattern, the WHOLE destination buffer compared with the expectation, and streams that carry an array to a decode call; for the
three filters with a capacity and a result per segment, the call that is compared with its reference as well (counted_call).  Each test file has
its own fixtures: seeds and sizes differ."""
import importlib.util
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402


def source(seed, size):
    """`size` seeded bytes, never changed"""
    a = np.random.default_rng(seed).integers(0, 256, size=size, dtype=np.uint8)
    a.setflags(write=False)
    return a


def sentinel(size):
    """what a destination buffer holds in front of a call: a pattern of period 251 (byte i is i % 251 + 3), so that no shifted copy of it is itself"""
    a = (np.arange(size, dtype=np.uint64) % 251 + 3).astype(np.uint8)
    a.setflags(write=False)
    return a


def device_buffers(source, sentinel):
    """the source and the sentinel on the device, and the one destination buffer, as large as the sentinel"""
    import torch
    d = {"src": torch.from_numpy(source.copy()).cuda(), "sentinel": torch.from_numpy(sentinel.copy()).cuda(),
         "dst": torch.empty(len(sentinel), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    assert d["src"].data_ptr() % 16 == 0 and d["dst"].data_ptr() % 16 == 0
    return d


def fresh_dst(dev, size):
    import torch
    assert size <= len(dev["dst"])
    dev["dst"][:size].copy_(dev["sentinel"][:size])
    torch.cuda.synchronize()


def compare(dev, want, segs=None, names="(src, dst, len, w)", dst_len=lambda s: s[2]):
    """the whole destination buffer against the expectation; names: what a segment's tuple holds; dst_len(segment): its destination's bytes"""
    got = dev["dst"][:len(want)].cpu().numpy()
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        inside = [s for s in (segs or []) if s[1] <= at < s[1] + dst_len(s)]
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %s: %r" %
                             (at, got[at], want[at], names, inside[:1] or "none: outside every segment"))


def upload(src):
    """bytes on the device, with 16 bytes of room behind them"""
    import torch
    t = torch.frombuffer(bytearray(src) + bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def pack(datas, start=3, gap=lambda i: i % 3):
    """segments' bytes one after the other in one source -> (source, [source offset])"""
    src, offs = bytearray(b"\xee" * start), []
    for i, d in enumerate(datas):
        src += b"\xee" * gap(i)
        offs.append(len(src))
        src += d
    return bytes(src), offs


def counted_call(call, elements_bytes, layout, dev, src, d_src, sentinel, segs, size):
    """One call of a filter with a capacity and a result per segment into a fresh destination of `size` bytes, the results compared item by item
    and the whole destination compared.  segs: [(source offset, source length, destination offset, cap, *columns)], the columns being what
    call(src_ptrs, src_lens, dst_ptrs, caps, *columns) -- a Batch's *_segments -- takes behind the capacities, and what the reference's
    elements_bytes(bytes, *columns, cap) -> (the elements' bytes, the result) takes between the bytes and the capacity.  layout: the names of
    what a segment's tuple holds, the width's being "w"; d_src: src on the device.  -> the results"""
    want, results = sentinel[:size].copy(), []
    for s, l, d, cap, *columns in segs:
        elems, res = elements_bytes(src[s:s + l], *columns, cap)
        assert d + len(elems) <= size
        want[d:d + len(elems)] = np.frombuffer(elems, dtype=np.uint8)
        results.append(res)
    fresh_dst(dev, size)
    sp, dp = d_src.data_ptr(), dev["dst"].data_ptr()
    got = call([sp + s[0] for s in segs], [s[1] for s in segs], [dp + s[2] for s in segs], [s[3] for s in segs],
               *[[s[k] for s in segs] for k in range(4, len(layout))])
    assert got == results, [(i, a, b) for i, (a, b) in enumerate(zip(got, results)) if a != b][:3]
    compare(dev, want, segs, names="(%s)" % ", ".join(layout), dst_len=lambda s: s[3] * s[layout.index("w")])
    return got


def next_at(at, align, mod=16):
    while at % mod != align:
        at += 1
    return at


def stream(raw):
    """a stream of stored metablocks and, where there are enough bytes, a compressed last one (tools/brotli_emit.py, as tests/size_streams.py)"""
    w = E.BitWriter(); E.write_stream_header(w, 22)
    if len(raw) < 64:
        if raw:
            E.emit_stored(w, raw)
        E.emit_last_empty(w)
        return w.finish()
    cut = len(raw) - min(1500, len(raw) // 2)
    head, tail = raw[:cut], raw[cut:]
    E.emit_stored(w, head[:len(head) // 2]); E.emit_stored(w, head[len(head) // 2:])
    got = E.emit_compressed(w, E.greedy_commands(tail, max_dist=1000, history=b""), E.Plan(), True, prev=head)
    assert got == tail
    return w.finish()


def slots(sizes, skip=(), start=5):
    """destinations back to back from offset `start` on -> ([offset or None], bytes in all)"""
    offs, at = [], start
    for i, n in enumerate(sizes):
        offs.append(None if i in skip else at)
        at += n
    return offs, at + 64


def tensors_module():
    """the package's tensors module, loaded once beside the package"""
    name = "rust_brotli_decompressor_amd.tensors"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "rust-brotli-decompressor_amd", "tensors.py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]
