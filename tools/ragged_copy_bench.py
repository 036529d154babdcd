#!/usr/bin/env python3
"""Throughput of the ragged copy kernel (csrc/brotli_copy_kernels.hip) through its test hook, for information: one 256 MiB segment against a
device-to-device copy of the same bytes by the runtime (torch's Tensor.copy_), and 4096 segments of 4 KiB at mixed alignments.

    python tools/ragged_copy_bench.py [--out FILE]

BrotliAmdDebugRaggedCopy allocates and uploads its segment table, launches and waits, so what is timed is the whole hook (host wall clock, the
median of eleven calls after two warm-up calls); the line 'hook alone' is the same call with one empty segment -- what the hook costs beside the kernel."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stream_sessions import load_pkg  # noqa: E402


def timed(fn, sync, reps=11):
    for _ in range(2):
        fn(); sync()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    L = pkg.load_library()
    sync = torch.cuda.synchronize
    big = 256 << 20
    src = torch.randint(0, 256, (big + 64,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros(big + 64, dtype=torch.uint8, device="cuda")

    def hook(segs):
        n = len(segs)
        s = (ctypes.c_void_p * n)(*[src.data_ptr() + x for x, _, _ in segs])
        d = (ctypes.c_void_p * n)(*[dst.data_ptr() + y for _, y, _ in segs])
        ln = (ctypes.c_size_t * n)(*[z for _, _, z in segs])
        return lambda: L.BrotliAmdDebugRaggedCopy(n, s, d, ln)

    lines = []

    def report(what, ms, nbytes):
        lines.append("%-64s %9.3f ms %s" % (what, ms, ("%8.1f GB/s copied" % (nbytes / ms / 1e6)) if nbytes else ""))
        print(lines[-1], flush=True)

    report("hook alone (one empty segment)", timed(hook([(0, 0, 0)]), sync), 0)
    report("ragged copy, one 256 MiB segment, both ends 16-byte aligned", timed(hook([(0, 0, big)]), sync), big)
    report("ragged copy, one 256 MiB segment, source + 3, destination + 5", timed(hook([(3, 5, big)]), sync), big)
    report("runtime device-to-device copy, 256 MiB", timed(lambda: dst[:big].copy_(src[:big]), sync), big)
    rnd = random.Random(5)
    segs, at = [], 0
    for i in range(4096):
        at += rnd.randrange(0, 16)
        segs.append((rnd.randrange(0, big - 4096), at, 4096))
        at += 4096
    report("ragged copy, 4096 x 4 KiB at mixed alignments", timed(hook(segs), sync), 4096 * 4096)
    ok = all(bytes(dst[y:y + z].cpu().numpy()) == bytes(src[x:x + z].cpu().numpy()) for x, y, z in segs[:64])
    lines.append("bytes of the first 64 segments: %s" % ("ok" if ok else "WRONG"))
    print(lines[-1])
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
