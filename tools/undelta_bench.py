#!/usr/bin/env python3
"""The undelta kernels (csrc/brotli_undelta_kernels.hip) against the ragged copy and against what a caller does without them, for DESIGN
section 8:

    python tools/undelta_bench.py [--out FILE] [--runs 10] [--rows metric,one64,one1g,small,tiny] [--widths 1,2,4,8]

Per row of segments in device memory, per placement and per width, three legs, taken IN TURNS (run k of each before run k + 1 of any), the
median of --runs runs after two warm-up runs of each:
  undelta  BrotliAmdBatchUndeltaSegments: the three launches' milliseconds together (BrotliAmdBatchLastUndeltaMs: HIP events around them), each
           phase's share of them (1: the tiles' sums, 2: the carries, 3: the running sums), GB/s of segment bytes over them, and the whole call
           as host wall time (table upload, launches, wait);
  copy     the ragged copy kernel moving the same segments device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall time, which
           allocates and uploads its table as well).  The copy reads and writes every byte once; undelta reads a long segment twice and writes
           it once.  Compare it with the undelta CALL, host wall against host wall;
  today    a loop of torch.cumsum(view, 0, dtype=...) over the segments whose address and length are multiples of the width (the others cannot
           be viewed as elements at all), as host wall time with a synchronize at the end, and the number of launches it took.
The long rows are placed twice: "packed" -- sources at an odd address, destinations 64-byte aligned, as a packed output gives them -- and
"odd dst" -- sources aligned, destinations at an odd address.  The short rows keep their own offsets for both.
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
PLACEMENTS = [("packed: odd src, 64-byte-aligned dst", 3, 0), ("odd dst, aligned src", 0, 5)]


def rows():
    """name -> (title, [(offset, length)], is it a long row): segments of one source buffer (the sets of tools/unshuffle_bench.py)"""
    rnd = random.Random(8)
    tiny, at = [], 0
    for _ in range(100000):
        at += rnd.randrange(0, 16)
        tiny.append((at, 100)); at += 100
    return {
        "metric": ("the metric's outputs: 256 x 4 MiB", [(i * 4 * MIB, 4 * MIB) for i in range(256)], True),
        "one64": ("one output of 64 MiB", [(0, 64 * MIB)], True),
        "one1g": ("one output of 1 GiB", [(0, 1024 * MIB)], True),
        "small": ("small documents: 4096 x 8 KiB", [(i * 8192, 8192) for i in range(4096)], False),
        "tiny": ("tiny segments: 100 000 x 100 B at mixed alignments", tiny, False),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="metric,one64,one1g,small,tiny")
    ap.add_argument("--widths", default="1,2,4,8")
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
    signed = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}   # (a wrapping sum has the same bits signed or not)
    pkg = load_pkg()
    L = pkg.load_library()
    sync = torch.cuda.synchronize
    room = max(o + l for name in names for o, l in table[name][1])
    src = torch.randint(0, 256, (room + 128,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(room + 128, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 64 == 0 and dst.data_ptr() % 64 == 0
    batch = pkg.Batch(1)

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    say("tile %d bytes, carry span %d tiles" % (pkg.undelta_tile(), pkg.undelta_carry_span()))
    ok = True
    for name in names:
        title, segs, long_row = table[name]
        n, nbytes = len(segs), sum(l for _, l in segs)
        a_len = (ctypes.c_size_t * n)(*[l for _, l in segs])
        for place, s_off, d_off in (PLACEMENTS if long_row else [("its own offsets", 0, 0)]):
            a_src = (ctypes.c_void_p * n)(*[src.data_ptr() + s_off + o for o, _ in segs])
            a_dst = (ctypes.c_void_p * n)(*[dst.data_ptr() + d_off + o for o, _ in segs])
            say("%s; %s (%d segments, %.1f MiB; median of %d)" % (title, place, n, nbytes / MIB, a.runs))
            for w in widths:
                a_w = (ctypes.c_uint8 * n)(*([w] * n))
                able = [(o, l) for o, l in segs if (s_off + o) % w == 0 and l % w == 0 and l]
                kept = {}

                def undelta():
                    t0 = time.perf_counter()
                    if L.BrotliAmdBatchUndeltaSegments(batch._h, n, a_src, a_dst, a_len, a_w, None) != 0:
                        raise RuntimeError(pkg.last_error())
                    wall = (time.perf_counter() - t0) * 1e3
                    return batch.last_undelta_ms(), wall, [batch.last_undelta_ms(p) for p in (1, 2, 3)]

                def copy():
                    t0 = time.perf_counter()
                    if L.BrotliAmdDebugRaggedCopy(n, a_src, a_dst, a_len) != 0:
                        raise RuntimeError(pkg.last_error())
                    return (time.perf_counter() - t0) * 1e3

                def today(keep):
                    t0 = time.perf_counter()
                    for k, (o, l) in enumerate(able):
                        t = torch.cumsum(src[s_off + o:s_off + o + l].view(signed[w]), 0, dtype=signed[w])
                        if keep and k < 64:
                            kept[o] = t
                    sync()
                    return (time.perf_counter() - t0) * 1e3

                kernel_ms, call_ms, copy_ms, today_ms, phase_ms = [], [], [], [], [[], [], []]
                same = None
                for run in range(-2, a.runs):
                    sync()
                    c = copy()
                    k, wall, ph = undelta()
                    if run == -2:
                        today(True)
                        if kept:
                            same = all(torch.equal(dst[d_off + o:d_off + o + t.numel() * w], t.view(torch.uint8)) for o, t in kept.items())
                            ok = ok and same
                        kept.clear()
                        continue
                    t = today(False)
                    if run >= 0:
                        kernel_ms.append(k); call_ms.append(wall); copy_ms.append(c); today_ms.append(t)
                        for p in range(3):
                            phase_ms[p].append(ph[p])
                k, wall, c, t = (statistics.median(v) for v in (kernel_ms, call_ms, copy_ms, today_ms))
                ph = [statistics.median(v) for v in phase_ms]
                gbs = lambda ms: nbytes / ms / 1e6   # noqa: E731
                able_bytes = sum(l for _, l in able)
                say("  width %d" % w)
                say("    undelta, three launches  %10.3f ms %9.1f GB/s   (phases 1 / 2 / 3: %.3f / %.3f / %.3f ms = %.0f / %.0f / %.0f %%)"
                    % (k, gbs(k), ph[0], ph[1], ph[2], 100 * ph[0] / k, 100 * ph[1] / k, 100 * ph[2] / k))
                say("    the call, host wall      %10.3f ms %9.1f GB/s   (%.2f x the copy's hook)" % (wall, gbs(wall), wall / c))
                say("    ragged copy, D2D         %10.3f ms %9.1f GB/s   (its hook, host wall)" % (c, gbs(c)))
                if able:
                    say("    today: torch.cumsum      %10.3f ms %9.1f GB/s   (host wall; %d launches for %d of the %d segments)"
                        % (t, able_bytes / t / 1e6, len(able), len(able), n))
                else:
                    say("    today: torch.cumsum      no segment can be viewed as elements of %d bytes here" % w)
                say("    equal to the loop's values: %s" % ("no segment to compare" if same is None else "yes" if same else "NO"))
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
