#!/usr/bin/env python3
"""The unshuffle kernel (csrc/brotli_unshuffle_kernels.hip) against the ragged copy and against what a caller does without it, for DESIGN
section 8:

    python tools/unshuffle_bench.py [--out FILE] [--runs 10] [--rows metric,one64,one1g,small,tiny] [--widths 2,4,8]

Per row of segments in device memory and per width, three legs, taken IN TURNS (run k of each before run k + 1 of any), the median of --runs
runs after two warm-up runs of each:
  unshuffle  BrotliAmdBatchUnshuffleSegments: the kernel's milliseconds (BrotliAmdBatchLastUnshuffleMs: HIP events around the launch), GB/s of
             segment bytes over them, and the whole call as host wall time (table upload, launch, wait);
  copy       the ragged copy kernel moving the same segments device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall time, which
             allocates and uploads its table as well): both kernels read and write every byte once, so the copy is the bandwidth yardstick --
             compare it with the unshuffle CALL, host wall against host wall;
  today      a loop of view(w, m).t().contiguous() over the segments whose offset and length are multiples of the width (the others cannot be
             viewed as elements at all), as host wall time with a synchronize at the end, and the number of launches it took.
The first run's destination is compared with the loop's results on the device (the first 64 segments that the loop can do)."""
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

MIB = 1 << 20


def rows():
    """name -> (title, [(offset, length)]): segments of one source buffer (the sets of tools/digest_bench.py)"""
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
    ap.add_argument("--widths", default="2,4,8")
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs: at least 1")
    table = rows()
    names = a.rows.split(",")
    for name in names:
        if name not in table:
            ap.error("--rows: one of " + ",".join(table))
    widths = [int(w) for w in a.widths.split(",")]
    if any(w not in (1, 2, 4, 8) for w in widths):
        ap.error("--widths: 1, 2, 4 or 8")
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

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    ok = True
    for name in names:
        title, segs = table[name]
        n, nbytes = len(segs), sum(l for _, l in segs)
        a_src = (ctypes.c_void_p * n)(*[src.data_ptr() + o for o, _ in segs])
        a_dst = (ctypes.c_void_p * n)(*[dst.data_ptr() + o for o, _ in segs])
        a_len = (ctypes.c_size_t * n)(*[l for _, l in segs])
        say("%s (%d segments, %.1f MiB; median of %d)" % (title, n, nbytes / MIB, a.runs))
        for w in widths:
            a_w = (ctypes.c_uint8 * n)(*([w] * n))
            able = [(o, l) for o, l in segs if o % w == 0 and l % w == 0 and l]
            kept = {}

            def unshuffle():
                t0 = time.perf_counter()
                if L.BrotliAmdBatchUnshuffleSegments(batch._h, n, a_src, a_dst, a_len, a_w, None) != 0:
                    raise RuntimeError(pkg.last_error())
                return batch.last_unshuffle_ms(), (time.perf_counter() - t0) * 1e3

            def copy():
                t0 = time.perf_counter()
                if L.BrotliAmdDebugRaggedCopy(n, a_src, a_dst, a_len) != 0:
                    raise RuntimeError(pkg.last_error())
                return (time.perf_counter() - t0) * 1e3

            def today(keep):
                t0 = time.perf_counter()
                for k, (o, l) in enumerate(able):
                    t = src[o:o + l].view(w, l // w).t().contiguous()
                    if keep and k < 64:
                        kept[o] = t
                sync()
                return (time.perf_counter() - t0) * 1e3

            kernel_ms, call_ms, copy_ms, today_ms = [], [], [], []
            same = True
            for run in range(-2, a.runs):
                sync()
                c = copy()
                k, wall = unshuffle()
                if run == -2:
                    today(True)
                    same = all(torch.equal(dst[o:o + t.numel()], t.reshape(-1)) for o, t in kept.items())
                    ok = ok and same
                    kept.clear()
                    continue
                t = today(False)
                if run >= 0:
                    kernel_ms.append(k); call_ms.append(wall); copy_ms.append(c); today_ms.append(t)
            k, wall, c, t = (statistics.median(v) for v in (kernel_ms, call_ms, copy_ms, today_ms))
            gbs = lambda ms: nbytes / ms / 1e6   # noqa: E731
            able_bytes = sum(l for _, l in able)
            say("  width %d" % w)
            say("    unshuffle kernel         %10.3f ms %9.1f GB/s   (the call, host wall: %.3f ms %9.1f GB/s)" % (k, gbs(k), wall, gbs(wall)))
            say("    ragged copy, D2D         %10.3f ms %9.1f GB/s   (its hook, host wall)" % (c, gbs(c)))
            say("    today: t().contiguous()  %10.3f ms %9.1f GB/s   (host wall; %d launches for %d of the %d segments)"
                % (t, able_bytes / t / 1e6, len(able), len(able), n))
            say("    equal to the loop's elements: %s" % ("yes" if same else "NO"))
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
