#!/usr/bin/env python3
"""The digest kernel (csrc/brotli_crc_kernels.hip) against what a caller does without it, for DESIGN section 8:

    python tools/digest_bench.py [--out FILE] [--runs 10] [--rows metric,one64,one1g,small,tiny]

Per row of segments in device memory, three legs, taken IN TURNS (run k of each before run k + 1 of any), the median of --runs runs after
two warm-up runs of each:
  digest   BrotliAmdBatchDigestSegments, CRC-32: the kernel's milliseconds (BrotliAmdBatchLastDigestMs: HIP events around the launch), GB/s
           of segment bytes over them, and the whole call as host wall time (table upload, launch, wait, digests back);
  today    a device-to-host copy of the same bytes and zlib.crc32 of every segment on one core, as host wall time;
  copy     the ragged copy kernel moving the same segments device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall time, which
           allocates and uploads its table as well) -- a bandwidth yardstick.
The digests of the first run are compared with zlib's."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stream_sessions import load_pkg  # noqa: E402

MIB = 1 << 20


def rows():
    """name -> (title, [(offset, length)]): segments of one source buffer"""
    rnd = random.Random(8)
    tiny, at = [], 0
    for _ in range(100000):
        at += rnd.randrange(0, 16)
        tiny.append((at, 100)); at += 100
    return {
        "metric": ("the metric's outputs: 256 x 4 MiB", [(i * 4 * MIB, 4 * MIB) for i in range(256)]),
        "one64": ("one output of 64 MiB", [(0, 64 * MIB)]),
        "one1g": ("one output of 1 GiB", [(0, 1024 * MIB)]),
        "small": ("small documents: 4096 x 8 KiB", [(i * 8192, 8192) for i in range(4096)]),
        "tiny": ("tiny segments: 100 000 x 100 B at mixed alignments", tiny),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="metric,one64,one1g,small,tiny")
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs: at least 1")
    table = rows()
    names = a.rows.split(",")
    for name in names:
        if name not in table:
            ap.error("--rows: one of " + ",".join(table))
    import torch
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    pkg = load_pkg()
    L = pkg.load_library()
    sync = torch.cuda.synchronize
    room = max(o + l for name in names for o, l in table[name][1])
    src = torch.randint(0, 256, (room + 64,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(room + 64, dtype=torch.uint8, device="cuda")
    batch = pkg.Batch(1)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    ok = True
    for name in names:
        title, segs = table[name]
        n, nbytes = len(segs), sum(l for _, l in segs)
        a_src = (ctypes.c_void_p * n)(*[src.data_ptr() + o for o, _ in segs])
        a_dst = (ctypes.c_void_p * n)(*[dst.data_ptr() + o for o, _ in segs])
        a_len = (ctypes.c_size_t * n)(*[l for _, l in segs])
        a_out = (ctypes.c_uint32 * n)()
        lo, hi = segs[0][0], max(o + l for o, l in segs)
        got = {}

        def digest():
            t0 = time.perf_counter()
            if L.BrotliAmdBatchDigestSegments(batch._h, pkg.DIGEST_CRC32, n, a_src, a_len, a_out, None) != 0:
                raise RuntimeError(pkg.last_error())
            wall = (time.perf_counter() - t0) * 1e3
            got["digest"] = list(a_out)
            return batch.last_digest_ms(), wall

        def today():
            t0 = time.perf_counter()
            host = memoryview(src[lo:hi].cpu().numpy())
            got["today"] = [zlib.crc32(host[o - lo:o - lo + l]) for o, l in segs]
            return (time.perf_counter() - t0) * 1e3

        def copy():
            t0 = time.perf_counter()
            if L.BrotliAmdDebugRaggedCopy(n, a_src, a_dst, a_len) != 0:
                raise RuntimeError(pkg.last_error())
            return (time.perf_counter() - t0) * 1e3

        kernel_ms, call_ms, today_ms, copy_ms = [], [], [], []
        for run in range(-2, a.runs):
            sync()
            k, w = digest()
            t = today()
            c = copy()
            if run == -2:
                same = got["digest"] == got["today"]
                ok = ok and same
            if run >= 0:
                kernel_ms.append(k); call_ms.append(w); today_ms.append(t); copy_ms.append(c)
        k, w, t, c = (statistics.median(v) for v in (kernel_ms, call_ms, today_ms, copy_ms))
        gbs = lambda ms: nbytes / ms / 1e6   # noqa: E731
        say("%s (%d segments, %.1f MiB; median of %d)" % (title, n, nbytes / MIB, a.runs))
        say("  digest kernel            %10.3f ms %9.1f GB/s   (the call, host wall: %.3f ms)" % (k, gbs(k), w))
        say("  today: D2H + zlib.crc32  %10.3f ms %9.1f GB/s   (host wall)" % (t, gbs(t)))
        say("  ragged copy, D2D         %10.3f ms %9.1f GB/s   (its hook, host wall)" % (c, gbs(c)))
        say("  digests equal zlib's: %s" % ("yes" if same else "NO"))
    batch.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
