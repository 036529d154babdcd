#!/usr/bin/env python3
"""The unrle kernels (csrc/brotli_unrle_kernels.hip) against the ragged copy, against the bit-unpack kernel and against what a caller does
without them, for DESIGN section 8:

    python tools/unrle_bench.py [--out FILE] [--runs 10] [--rows pages,short,one64,tiny]

Per row of segments in device memory -- runs of Parquet's RLE / bit-packed hybrid with fields of 12 bits into elements of 4 bytes --, four legs,
taken IN TURNS (run k of each before run k + 1 of any), the median of --runs runs after two warm-up runs of each:
  unrle     BrotliAmdBatchUnrleSegments with capacities from a counting call: the two launches' milliseconds together (BrotliAmdBatchLastUnrleMs:
            HIP events around them), each phase's (1: the walk, 2: the expansion), GB/s of DESTINATION bytes over them, and the whole call as
            host wall time (table upload, launches, wait, results);
  copy      the ragged copy kernel moving the same DESTINATION bytes device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall
            time, which allocates and uploads its table as well): what writing that many bytes costs;
  unpack    the bit-unpack kernel (BrotliAmdBatchLastBitUnpackMs of a BrotliAmdBatchBitUnpackSegments call) at the same field and element widths
            over the same number of values a segment, each segment's input being one bit-packed run's payload: the expansion without runs;
  today     a device-to-host copy of the source and the numpy reference (tests/rle_ref.py) over it, as host wall time, ONE run, over at most the
            first --today-mib MiB of the row's destinations (the rate is what is compared).
The rows: "pages" 1024 segments of 64 Ki values, seeded runs of 8 .. 504 packed and 8 .. 2000 repeated values; "short" the same with every run 8
values; "one64" one segment of 64 MiB of destination; "tiny" 100 000 segments of 40 values at mixed alignments.  A row's segments are drawn from
sixteen (tiny: sixty-four) seeded ones, over and over.  The first run's results and elements of the first segments are compared with the reference."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stream_sessions import load_pkg  # noqa: E402
import rle_ref as ref  # noqa: E402

MIB = 1 << 20
K, W = 12, 4


def segment(rng, values, packed, repeated):
    """seeded runs that hold at least `values` values: packed ones of packed[0] .. packed[1] values (multiples of 8; None: none), repeated
    ones of repeated[0] .. repeated[1] (None: none); the fields are seeded bits -> bytes"""
    out, have = [], 0
    while have < values:
        if repeated is None or (packed is not None and rng.integers(2)):
            g = int(rng.integers(packed[0] // 8, packed[1] // 8 + 1))
            out.append(ref.header(g << 1 | 1) + rng.integers(0, 256, size=g * K, dtype=np.uint8).tobytes())
            have += 8 * g
        else:
            c = int(rng.integers(repeated[0], repeated[1] + 1))
            out.append(ref.header(c << 1) + int(rng.integers(0, 1 << K)).to_bytes((K + 7) // 8, "little"))
            have += c
    return b"".join(out)


ROWS = {   # name -> (title, segments, values a segment, distinct segments, packed, repeated, mixed alignments)
    "pages": ("1024 pages of 64 Ki values, runs of 8 .. 504 packed and 8 .. 2000 repeated", 1024, 1 << 16, 16, (8, 504), (8, 2000), False),
    "short": ("1024 pages of 64 Ki values, every run 8 values", 1024, 1 << 16, 16, (8, 8), (8, 8), False),
    "one64": ("one segment of 64 MiB of destination", 1, 64 * MIB // W, 1, (8, 504), (8, 2000), False),
    "tiny": ("tiny segments: 100 000 x 40 values at mixed alignments", 100000, 40, 64, (8, 16), (1, 12), True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="pages,short,one64,tiny")
    ap.add_argument("--today-mib", type=int, default=16)
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs: at least 1")
    names = a.rows.split(",")
    for name in names:
        if name not in ROWS:
            ap.error("--rows: one of " + ",".join(ROWS))
    import torch
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    pkg = load_pkg()
    L = pkg.load_library()
    sync = torch.cuda.synchronize
    batch = pkg.Batch(1)

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    say("item %d elements, walk chunk %d bytes; fields of %d bits into elements of %d bytes" % (pkg.unrle_item_elems(), pkg.unrle_walk_chunk(), K, W))
    ok = True
    for name in names:
        title, n, values, distinct, packed, repeated, mixed = ROWS[name]
        rng = np.random.default_rng(20280)
        kinds = [segment(rng, values, packed, repeated) for _ in range(distinct)]
        # the source: the segments one after the other, the tiny ones at mixed alignments
        offs, lens, at = [], [], 0
        for i in range(n):
            at += i % 5 if mixed else 0
            offs.append(at); lens.append(len(kinds[i % distinct]))
            at += lens[-1]
        host = np.zeros(at + 16, dtype=np.uint8)
        for i in range(n):
            host[offs[i]:offs[i] + lens[i]] = np.frombuffer(kinds[i % distinct], dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        sync()
        sp = src.data_ptr()
        a_src = (ctypes.c_void_p * n)(*[sp + o for o in offs])
        a_len = (ctypes.c_size_t * n)(*lens)
        counted = batch.unrle_segments([sp + o for o in offs], lens, None, [0] * n, [K] * n, [W] * n)
        count_ms = batch.last_unrle_ms()
        total, runs = sum(r[0] for r in counted), sum(r[2] for r in counted)
        say("%s (%d segments, %.1f MiB of source, %d values in %d runs, %.1f MiB of elements; counting alone %.3f ms; median of %d)"
            % (title, n, sum(lens) / MIB, total, runs, total * W / MIB, count_ms, a.runs))
        if any(r[3] != ref.OK for r in counted):
            say("  a segment did not end well: %r" % ([r for r in counted if r[3] != ref.OK][:3],))
            ok = False
            continue
        d_offs, at = [], 0
        for i, r in enumerate(counted):
            at += i % 7 if mixed else 0
            d_offs.append(at)
            at += r[0] * W
        out_bytes = total * W
        dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
        fields = torch.randint(0, 256, ((total * K + 7) // 8 + n + 128,), dtype=torch.uint8, device="cuda")   # every segment's one packed run
        f_offs, f_at = [], 0
        for r in counted:
            f_offs.append(f_at)
            f_at += (r[0] * K + 7) // 8
        dp = dst.data_ptr()
        a_dst = (ctypes.c_void_p * n)(*[dp + o for o in d_offs])
        a_cap = (ctypes.c_uint64 * n)(*[r[0] for r in counted])
        a_k = (ctypes.c_uint8 * n)(*([K] * n))
        a_w = (ctypes.c_uint8 * n)(*([W] * n))
        a_cdst = (ctypes.c_void_p * n)(*[copy_dst.data_ptr() + o for o in d_offs])
        a_clen = (ctypes.c_size_t * n)(*[r[0] * W for r in counted])
        a_fsrc = (ctypes.c_void_p * n)(*[fields.data_ptr() + o for o in f_offs])
        a_flen = (ctypes.c_size_t * n)(*[(r[0] * K + 7) // 8 for r in counted])
        res = (pkg.UnrleResult * n)()

        def unrle():
            t0 = time.perf_counter()
            if L.BrotliAmdBatchUnrleSegments(batch._h, n, a_src, a_len, a_dst, a_cap, a_k, a_w, None, res, None) != 0:
                raise RuntimeError(pkg.last_error())
            wall = (time.perf_counter() - t0) * 1e3
            return batch.last_unrle_ms(), wall, [batch.last_unrle_ms(p) for p in (1, 2)]

        def copy():
            t0 = time.perf_counter()
            if L.BrotliAmdDebugRaggedCopy(n, a_dst, a_cdst, a_clen) != 0:
                raise RuntimeError(pkg.last_error())
            return (time.perf_counter() - t0) * 1e3

        def unpack():
            if L.BrotliAmdBatchBitUnpackSegments(batch._h, n, a_fsrc, a_flen, a_cdst, a_cap, a_k, a_w, None, None) != 0:
                raise RuntimeError(pkg.last_error())
            return batch.last_bitunpack_ms()

        kernel_ms, call_ms, copy_ms, unpack_ms, phase_ms = [], [], [], [], [[], []]
        same, checked = True, 0
        for run in range(-2, a.runs):
            sync()
            k, wall, ph = unrle()
            c = copy()
            u = unpack()
            if run == -2:   # the first segments against the reference
                for i in range(min(n, 40)):
                    if counted[i][0] > 32 * MIB:
                        continue
                    elems, want = ref.elements_bytes(kinds[i % distinct], K, W, 0, counted[i][0])
                    got = dst[d_offs[i]:d_offs[i] + counted[i][0] * W].cpu().numpy().tobytes()
                    same = same and got == elems and res[i].astuple() == want == counted[i]
                    checked += 1
                ok = ok and same
            if run >= 0:
                kernel_ms.append(k); call_ms.append(wall); copy_ms.append(c); unpack_ms.append(u)
                for p in range(2):
                    phase_ms[p].append(ph[p])
        # today: the bytes to the host, and the reference over them
        upto, took = 0, 0
        for i in range(n):
            if took + counted[i][0] * W > a.today_mib * MIB and took:
                break
            upto += 1; took += counted[i][0] * W
        t0 = time.perf_counter()
        back = src[:offs[upto - 1] + lens[upto - 1]].cpu().numpy()
        for i in range(upto):
            ref.decode(back[offs[i]:offs[i] + lens[i]], K, W)
        today = (time.perf_counter() - t0) * 1e3
        k, wall, c, u = (statistics.median(v) for v in (kernel_ms, call_ms, copy_ms, unpack_ms))
        ph = [statistics.median(v) for v in phase_ms]
        gbs = lambda b, ms: b / ms / 1e6   # noqa: E731
        say("    unrle, two launches      %10.3f ms %8.1f GB/s of elements   (phases 1 / 2: %.3f / %.3f ms = %.0f / %.0f %%; %.1f ns a run in the walk)"
            % (k, gbs(out_bytes, k), ph[0], ph[1], 100 * ph[0] / k, 100 * ph[1] / k, 1e6 * ph[0] / max(1, runs)))
        say("    the call, host wall      %10.3f ms %8.1f GB/s of elements" % (wall, gbs(out_bytes, wall)))
        say("    ragged copy of the elements %7.3f ms %8.1f GB/s of elements   (its hook, host wall; phase 2 is %.2f x this)" % (c, gbs(out_bytes, c), ph[1] / c))
        say("    bit-unpack of as many fields %6.3f ms %8.1f GB/s of elements   (its kernel; phase 2 is %.2f x this)" % (u, gbs(out_bytes, u), ph[1] / u))
        say("    today: to the host and numpy %8.1f ms %8.3f GB/s of elements   (host wall, one run over %.1f MiB of %d segments)"
            % (today, gbs(took, today), took / MIB, upto))
        say("    equal to the reference: %s" % ("no segment short enough to compare" if not checked else "yes" if same else "NO"))
        del dst, copy_dst, fields, src
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
