#!/usr/bin/env python3
"""The bit-unpack kernel (csrc/brotli_bitunpack_kernels.hip) against the ragged copy over the same destination bytes, against the unshuffle kernel
at the same width and against what a caller does without it, for DESIGN section 8:

    python tools/bitunpack_bench.py [--out FILE] [--runs 10] [--rows metric,one64,small,tiny] [--shapes 1:1,4:1,7:1,12:2,20:4,40:8] [--today-mib 64] [--today-cap 256]

A row is a set of DESTINATION segments in device memory (the sets of tools/unshuffle_bench.py); under a shape k:w a segment of len bytes takes
len / w fields of k bits, LSB-first and zero-extended (7:1 and 40:8 also run MSB-first and signed), from ceil(len k / (8 w)) source bytes.
Four legs, taken IN TURNS (run r of each before run r + 1 of any), the median of --runs runs after two warm-up runs of each:
  bitunpack  BrotliAmdBatchBitUnpackSegments: the kernel's milliseconds (BrotliAmdBatchLastBitUnpackMs: HIP events around the launch), GB/s of
             DESTINATION bytes over them (and of source + destination bytes: what the kernel moves), and the whole call as host wall time;
  copy       the ragged copy kernel moving as many bytes as the destination has, device to device (BrotliAmdDebugRaggedCopy: its whole hook
             as host wall time, which allocates and uploads its table as well): compare it with the bit-unpack CALL, host wall against host wall;
  unshuffle  BrotliAmdBatchUnshuffleSegments over the same destination segments at the same width: kernel milliseconds and the call's host
             wall.  Same stores, as many bytes in as out, no bit arithmetic;
  today      a loop of torch bit operations over the first --today-cap segments whose offset is a multiple of the width, --today-mib of
             destination at the most (shift, mask, reshape, weighted sum; long segments in pieces, so that the temporaries stay small), as host wall time
             with a synchronize at the end, and the number of segments it did.
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
PIECE = 1 << 20   # elements the loop takes at a time (a multiple of 8: a piece begins at a byte); its temporaries are 8 k bytes an element
DTYPES = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def torch_bitunpack(torch, src, m, k, w, flags):
    """m fields of k bits in the uint8 tensor `src` -> the elements' bytes (a uint8 tensor of m w), by torch operations"""
    out = torch.empty(m * w, dtype=torch.uint8, device=src.device)
    msb, signed = bool(flags & 1), bool(flags & 2)
    shifts = torch.arange(8, dtype=torch.uint8, device=src.device)
    if msb:
        shifts = 7 - shifts
    place = torch.arange(k, dtype=torch.int64, device=src.device)
    if msb:
        place = k - 1 - place
    for e0 in range(0, m, PIECE):
        n = min(PIECE, m - e0)
        part = src[e0 * k // 8:(e0 * k + n * k + 7) // 8]
        bits = ((part.unsqueeze(-1) >> shifts) & 1).reshape(-1)[:n * k].reshape(n, k).to(torch.int64)
        v = (bits << place).sum(-1)
        if signed and k < 64:
            v = (v ^ (1 << (k - 1))) - (1 << (k - 1))
        out[e0 * w:(e0 + n) * w] = v.to(getattr(torch, DTYPES[w])).view(torch.uint8).reshape(-1) if w < 8 else v.view(torch.uint8).reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="metric,one64,small,tiny")
    ap.add_argument("--shapes", default="1:1,4:1,7:1,12:2,20:4,40:8")
    ap.add_argument("--today-mib", type=int, default=64)
    ap.add_argument("--today-cap", type=int, default=256)
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs: at least 1")
    table = rows()
    names = a.rows.split(",")
    for name in names:
        if name not in table:
            ap.error("--rows: one of " + ",".join(table))
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    if any(w not in (1, 2, 4, 8) or not 1 <= k <= 8 * w for k, w in shapes):
        ap.error("--shapes: k:w with w of 1, 2, 4 or 8 and k of 1 .. 8 w")
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
        say("%s (%d segments, %.1f MiB of destination; median of %d)" % (title, n, nbytes / MIB, a.runs))
        for k, w in shapes:
            a_w = (ctypes.c_uint8 * n)(*([w] * n))
            a_k = (ctypes.c_uint8 * n)(*([k] * n))
            counts = [l // w for _, l in segs]
            a_cnt = (ctypes.c_uint64 * n)(*counts)
            a_slen = (ctypes.c_size_t * n)(*[(m * k + 7) // 8 for m in counts])   # (a segment's source begins where its destination does: k <= 8 w)
            src_bytes = sum((m * k + 7) // 8 for m in counts)
            able, left = [], a.today_mib * MIB
            for (o, l), m in zip(segs, counts):
                if o % w == 0 and min(m, left // w) and len(able) < a.today_cap:
                    able.append((o, min(m, left // w)))
                    left -= able[-1][1] * w
            for flags in ((0, 3) if (k, w) in ((7, 1), (40, 8)) else (0,)):
                a_f = (ctypes.c_uint8 * n)(*([flags] * n))
                kept = {}

                def bitunpack():
                    t0 = time.perf_counter()
                    if L.BrotliAmdBatchBitUnpackSegments(batch._h, n, a_src, a_slen, a_dst, a_cnt, a_k, a_w, a_f, None) != 0:
                        raise RuntimeError(pkg.last_error())
                    return batch.last_bitunpack_ms(), (time.perf_counter() - t0) * 1e3

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
                    for i, (o, m) in enumerate(able):
                        t = torch_bitunpack(torch, src[o:o + (m * k + 7) // 8], m, k, w, flags)
                        if keep and i < 16:
                            kept[o] = t
                    sync()
                    return (time.perf_counter() - t0) * 1e3

                un_k, un_wall, copy_ms, sh_ms, sh_wall, today_ms = [], [], [], [], [], []
                same = True
                for run in range(-2, a.runs):
                    sync()
                    c = copy()
                    u, uwall = unshuffle()
                    p, wall = bitunpack()   # (the last writer of dst: what the comparison below reads)
                    if run == -2:
                        today(True)
                        same = all(torch.equal(dst[o:o + t.numel()], t) for o, t in kept.items())
                        ok = ok and same
                        kept.clear()
                        continue
                    t = today(False)
                    if run >= 0:
                        un_k.append(p); un_wall.append(wall); copy_ms.append(c); sh_ms.append(u); sh_wall.append(uwall); today_ms.append(t)
                p, wall, c, u, uwall, t = (statistics.median(v) for v in (un_k, un_wall, copy_ms, sh_ms, sh_wall, today_ms))
                gbs = lambda ms, b=nbytes: b / ms / 1e6   # noqa: E731
                able_bytes = sum(m * w for _, m in able)
                say("  k %d into width %d, %s" % (k, w, "MSB-first, signed" if flags else "LSB-first, unsigned"))
                say("    bit-unpack kernel        %10.3f ms %9.1f GB/s of destination, %9.1f GB/s read + written   (the call, host wall: %.3f ms %9.1f GB/s)"
                    % (p, gbs(p), gbs(p, nbytes + src_bytes), wall, gbs(wall)))
                say("    ragged copy, D2D         %10.3f ms %9.1f GB/s   (its hook, host wall)" % (c, gbs(c)))
                say("    unshuffle kernel         %10.3f ms %9.1f GB/s   (the call, host wall: %.3f ms %9.1f GB/s)" % (u, gbs(u), uwall, gbs(uwall)))
                say("    today: torch bit ops     %10.3f ms %9.1f GB/s   (host wall; %d of the %d segments, %.1f MiB of destination)"
                    % (t, able_bytes / t / 1e6, len(able), n, able_bytes / MIB))
                say("    kernel / unshuffle kernel: %.2f   call / copy hook: %.2f   equal to the loop's elements: %s" % (p / u, wall / c, "yes" if same else "NO"))
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
