#!/usr/bin/env python3
"""The bit-unshuffle kernel (csrc/brotli_bitunshuffle_kernels.hip) against the ragged copy, against the unshuffle kernel at the same width and
against what a caller does without it, for DESIGN section 8:

    python tools/bitunshuffle_bench.py [--out FILE] [--runs 5] [--rows metric,one64,one1g,small,tiny] [--widths 1,2,4,8] [--today-cap 256]

Per row of segments in device memory, per width and per block size (0: one block a segment; 8192 / w: the bitshuffle library's default), four
legs, taken IN TURNS (run k of each before run k + 1 of any), the median of --runs runs after two warm-up runs of each:
  bitunshuffle  BrotliAmdBatchBitUnshuffleSegments: the kernel's milliseconds (BrotliAmdBatchLastBitUnshuffleMs: HIP events around the launch), GB/s
                of segment bytes over them, and the whole call as host wall time (table upload, launch, wait);
  copy          the ragged copy kernel moving the same segments device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall time,
                which allocates and uploads its table as well): compare it with the bit-unshuffle CALL, host wall against host wall;
  unshuffle     BrotliAmdBatchUnshuffleSegments over the same segments at the same width: kernel milliseconds and the call's host wall.  Same
                bytes, same stores, without the bit transposes: the natural yardstick;
  today         a loop of torch bit operations over the first --today-cap segments whose offset and length are multiples of the width (shift,
                mask, transpose, shift, sum; long segments in pieces, so that the temporaries stay small), as host wall time with a
                synchronize at the end, and the number of segments it did.
The first run's destination is compared with the loop's results on the device (the first 16 segments that the loop can do)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stream_sessions import load_pkg  # noqa: E402
from unshuffle_bench import rows  # noqa: E402

MIB = 1 << 20
PIECE = 4 * MIB   # bytes of one bit row the loop takes at a time: its temporaries are 8 x 8 w times that


def torch_bitunshuffle(torch, seg, w, block):
    """the bit planes in the uint8 tensor `seg` (a multiple of w bytes) -> its elements' bytes, by torch operations"""
    m = seg.numel() // w
    out = seg.clone()
    shifts = torch.arange(8, dtype=torch.uint8, device=seg.device)
    spans = [(0, m // 8 * 8)] if block == 0 or block >= m else [(b0, block if m - b0 >= block else (m - b0) // 8 * 8) for b0 in range(0, m, block)]
    nb = 0 if block == 0 or block >= m else m // block
    if nb:   # the full blocks at once, a few at a time
        per = max(1, PIECE * 8 // block)
        for b0 in range(0, nb, per):
            k = min(per, nb - b0)
            rows_ = seg[b0 * block * w:(b0 + k) * block * w].view(k, 8 * w, block // 8)
            bits = ((rows_.unsqueeze(-1) >> shifts) & 1).reshape(k, 8 * w, block)            # [b, 8 j + k, i]
            vals = (bits.transpose(1, 2).reshape(k, block, w, 8) << shifts).sum(-1, dtype=torch.uint8)
            out[b0 * block * w:(b0 + k) * block * w] = vals.reshape(-1)
        spans = spans[nb:]
    for b0, c in spans:
        if c == 0:
            continue
        rows_ = seg[b0 * w:(b0 + c) * w].view(8 * w, c // 8)
        for c0 in range(0, c // 8, PIECE):
            part = rows_[:, c0:c0 + PIECE]
            n = part.shape[1] * 8
            bits = ((part.unsqueeze(-1) >> shifts) & 1).reshape(8 * w, n)
            vals = (bits.t().reshape(n, w, 8) << shifts).sum(-1, dtype=torch.uint8)
            out[(b0 + 8 * c0) * w:(b0 + 8 * c0 + n) * w] = vals.reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", default="metric,one64,one1g,small,tiny")
    ap.add_argument("--widths", default="1,2,4,8")
    ap.add_argument("--today-cap", type=int, default=256)
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
            able = [(o, l) for o, l in segs if o % w == 0 and l % w == 0 and l][:a.today_cap]
            for block in (0, 8192 // w):
                a_b = (ctypes.c_uint32 * n)(*([block] * n))
                kept = {}

                def bitunshuffle():
                    t0 = time.perf_counter()
                    if L.BrotliAmdBatchBitUnshuffleSegments(batch._h, n, a_src, a_dst, a_len, a_w, a_b, None) != 0:
                        raise RuntimeError(pkg.last_error())
                    return batch.last_bitunshuffle_ms(), (time.perf_counter() - t0) * 1e3

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
                        t = torch_bitunshuffle(torch, src[o:o + l], w, block)
                        if keep and k < 16:
                            kept[o] = t
                    sync()
                    return (time.perf_counter() - t0) * 1e3

                bit_ms, bit_wall, copy_ms, un_ms, un_wall, today_ms = [], [], [], [], [], []
                same = True
                for run in range(-2, a.runs):
                    sync()
                    c = copy()
                    u, uwall = unshuffle()
                    k, wall = bitunshuffle()   # (the last writer of dst: what the comparison below reads)
                    if run == -2:
                        today(True)
                        same = all(torch.equal(dst[o:o + t.numel()], t) for o, t in kept.items())
                        ok = ok and same
                        kept.clear()
                        continue
                    t = today(False)
                    if run >= 0:
                        bit_ms.append(k); bit_wall.append(wall); copy_ms.append(c); un_ms.append(u); un_wall.append(uwall); today_ms.append(t)
                k, wall, c, u, uwall, t = (statistics.median(v) for v in (bit_ms, bit_wall, copy_ms, un_ms, un_wall, today_ms))
                gbs = lambda ms: nbytes / ms / 1e6   # noqa: E731
                able_bytes = sum(l for _, l in able)
                say("  width %d, block %d" % (w, block))
                say("    bit-unshuffle kernel     %10.3f ms %9.1f GB/s   (the call, host wall: %.3f ms %9.1f GB/s)" % (k, gbs(k), wall, gbs(wall)))
                say("    ragged copy, D2D         %10.3f ms %9.1f GB/s   (its hook, host wall)" % (c, gbs(c)))
                say("    unshuffle kernel         %10.3f ms %9.1f GB/s   (the call, host wall: %.3f ms %9.1f GB/s)" % (u, gbs(u), uwall, gbs(uwall)))
                say("    today: torch bit ops     %10.3f ms %9.1f GB/s   (host wall; %d of the %d segments, %.1f MiB)"
                    % (t, able_bytes / t / 1e6, len(able), n, able_bytes / MIB))
                say("    kernel / unshuffle kernel: %.2f   call / copy hook: %.2f   equal to the loop's elements: %s" % (k / u, wall / c, "yes" if same else "NO"))
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
