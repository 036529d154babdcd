#!/usr/bin/env python3
"""The undbp kernels (csrc/brotli_undbp_kernels.hip) against the ragged copy, against bit-unpack followed by undelta and against what a caller
does without them, for DESIGN section 8:

    python tools/undbp_bench.py [--out FILE] [--runs 10] [--rows pages,narrow,one64,tiny]

Per row of segments in device memory -- DELTA_BINARY_PACKED streams of B = 128, M = 4 into elements of 8 bytes --, four legs, taken IN TURNS (run
k of each before run k + 1 of any), the median of --runs runs after two warm-up runs of each:
  undbp     BrotliAmdBatchUndbpSegments with capacities from a counting call: the four launches' milliseconds together (BrotliAmdBatchLastUndbpMs:
            HIP events around them), each phase's (1: the walk, 2: the items' sums, 3: the carries, 4: the expansion), GB/s of DESTINATION bytes
            over them, the walk's cost a block, and the whole call as host wall time (table upload, launches, wait, results);
  copy      the ragged copy kernel moving the same DESTINATION bytes device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall
            time, which allocates and uploads its table as well): what writing that many bytes costs;
  pipeline  the bit-unpack kernel over as many fields of the row's mean width into the same elements, then the undelta kernels over those
            elements (BrotliAmdBatchLastBitUnpackMs + BrotliAmdBatchLastUndeltaMs): what a caller could launch if it already knew where the
            blocks lie;
  today     a device-to-host copy of the source and the numpy reference (tests/dbp_ref.py) over it, as host wall time, ONE run, over at most the
            first --today-mib MiB of the row's destinations (the rate is what is compared).
The rows: "pages" 1024 segments of 64 Ki values, every miniblock's width seeded in 4 .. 20; "narrow" the same with widths 0 .. 4, where the walk
dominates; "one64" one segment of 64 MiB of destination, widths 4 .. 20; "tiny" 100 000 segments of 40 values at mixed alignments.  A row's
segments are drawn from sixteen (tiny: sixty-four) seeded ones, over and over; payloads are seeded bytes.  The first run's results and elements
of the first segments are compared with the reference."""
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
import dbp_ref as ref  # noqa: E402

MIB = 1 << 20
B, M, W = 128, 4, 8
V = B // M


def segment(rng, values, widths):
    """a stream of `values` values: every block a seeded min_delta, every needed miniblock a width seeded in widths[0] .. widths[1] and a
    payload of seeded bytes -> bytes"""
    out = [ref.varint(B), ref.varint(M), ref.varint(values), ref.varint(ref.zigzag(int(rng.integers(-1 << 40, 1 << 40))))]
    left = values - 1
    while left > 0:
        need = min(M, (min(left, B) + V - 1) // V)
        ks = [int(k) for k in rng.integers(widths[0], widths[1] + 1, size=need)]
        out.append(ref.varint(ref.zigzag(int(rng.integers(-50, 50)))) + bytes(ks + [0] * (M - need)))
        out.append(rng.integers(0, 256, size=sum(ks) * V // 8, dtype=np.uint8).tobytes())
        left -= min(left, B)
    return b"".join(out)


ROWS = {   # name -> (title, segments, values a segment, distinct segments, widths, bit-unpack's k, mixed alignments)
    "pages": ("1024 pages of 64 Ki INT64 values, widths 4 .. 20", 1024, 1 << 16, 16, (4, 20), 12, False),
    "narrow": ("1024 pages of 64 Ki INT64 values, widths 0 .. 4", 1024, 1 << 16, 16, (0, 4), 2, False),
    "one64": ("one segment of 64 MiB of destination, widths 4 .. 20", 1, 64 * MIB // W, 1, (4, 20), 12, False),
    "tiny": ("tiny segments: 100 000 x 40 values at mixed alignments, widths 0 .. 12", 100000, 40, 64, (0, 12), 6, True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="pages,narrow,one64,tiny")
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

    say("item %d deltas, walk chunk %d bytes; blocks of %d values in %d miniblocks into elements of %d bytes" % (pkg.undbp_item_deltas(), pkg.undbp_walk_chunk(), B, M, W))
    ok = True
    for name in names:
        title, n, values, distinct, widths, K, mixed = ROWS[name]
        rng = np.random.default_rng(20281)
        kinds = [segment(rng, values, widths) for _ in range(distinct)]
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
        counted = batch.undbp_segments([sp + o for o in offs], lens, None, [0] * n, [W] * n)
        count_ms = batch.last_undbp_ms()
        total, blocks = sum(r[0] for r in counted), sum(r[3] for r in counted)
        say("%s (%d segments, %.1f MiB of source, %d values in %d blocks, %.1f MiB of elements; counting alone %.3f ms; median of %d)"
            % (title, n, sum(lens) / MIB, total, blocks, total * W / MIB, count_ms, a.runs))
        if any(r[4] != ref.OK or r[1] != l for r, l in zip(counted, lens)):
            say("  a segment did not end well: %r" % ([r for r in counted if r[4] != ref.OK][:3],))
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
        sum_dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
        fields = torch.randint(0, 256, ((total * K + 7) // 8 + n + 128,), dtype=torch.uint8, device="cuda")   # every segment's fields, one width
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
        a_sdst = (ctypes.c_void_p * n)(*[sum_dst.data_ptr() + o for o in d_offs])
        a_clen = (ctypes.c_size_t * n)(*[r[0] * W for r in counted])
        a_fsrc = (ctypes.c_void_p * n)(*[fields.data_ptr() + o for o in f_offs])
        a_flen = (ctypes.c_size_t * n)(*[(r[0] * K + 7) // 8 for r in counted])
        res = (pkg.UndbpResult * n)()

        def undbp():
            t0 = time.perf_counter()
            if L.BrotliAmdBatchUndbpSegments(batch._h, n, a_src, a_len, a_dst, a_cap, a_w, None, res, None) != 0:
                raise RuntimeError(pkg.last_error())
            wall = (time.perf_counter() - t0) * 1e3
            return batch.last_undbp_ms(), wall, [batch.last_undbp_ms(p) for p in (1, 2, 3, 4)]

        def copy():
            t0 = time.perf_counter()
            if L.BrotliAmdDebugRaggedCopy(n, a_dst, a_cdst, a_clen) != 0:
                raise RuntimeError(pkg.last_error())
            return (time.perf_counter() - t0) * 1e3

        def pipeline():
            if L.BrotliAmdBatchBitUnpackSegments(batch._h, n, a_fsrc, a_flen, a_cdst, a_cap, a_k, a_w, None, None) != 0:
                raise RuntimeError(pkg.last_error())
            if L.BrotliAmdBatchUndeltaSegments(batch._h, n, a_cdst, a_sdst, a_clen, a_w, None) != 0:
                raise RuntimeError(pkg.last_error())
            return batch.last_bitunpack_ms() + batch.last_undelta_ms()

        kernel_ms, call_ms, copy_ms, pipe_ms, phase_ms = [], [], [], [], [[], [], [], []]
        same, checked = True, 0
        for run in range(-2, a.runs):
            sync()
            k, wall, ph = undbp()
            c = copy()
            u = pipeline()
            if run == -2:   # the first segments against the reference
                for i in range(min(n, 40)):
                    if counted[i][0] * W > 64 * MIB:
                        continue
                    elems, want = ref.elements_bytes(kinds[i % distinct], W, counted[i][0])
                    got = dst[d_offs[i]:d_offs[i] + counted[i][0] * W].cpu().numpy().tobytes()
                    same = same and got == elems and res[i].astuple() == want == counted[i]
                    checked += 1
                ok = ok and same
            if run >= 0:
                kernel_ms.append(k); call_ms.append(wall); copy_ms.append(c); pipe_ms.append(u)
                for p in range(4):
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
            ref.decode(back[offs[i]:offs[i] + lens[i]].tobytes(), W)
        today = (time.perf_counter() - t0) * 1e3
        k, wall, c, u = (statistics.median(v) for v in (kernel_ms, call_ms, copy_ms, pipe_ms))
        ph = [statistics.median(v) for v in phase_ms]
        gbs = lambda b, ms: b / ms / 1e6   # noqa: E731
        say("    undbp, four launches     %10.3f ms %8.1f GB/s of elements   (phases 1 / 2 / 3 / 4: %.3f / %.3f / %.3f / %.3f ms = %.0f / %.0f / %.0f / %.0f %%; %.1f ns a block in the walk)"
            % ((k, gbs(out_bytes, k)) + tuple(ph) + tuple(100 * p / k for p in ph) + (1e6 * ph[0] / max(1, blocks),)))
        say("    the call, host wall      %10.3f ms %8.1f GB/s of elements" % (wall, gbs(out_bytes, wall)))
        say("    ragged copy of the elements %7.3f ms %8.1f GB/s of elements   (its hook, host wall; the call's kernels are %.2f x this)" % (c, gbs(out_bytes, c), k / c))
        say("    bit-unpack, then undelta %10.3f ms %8.1f GB/s of elements   (their kernels, fields of %d bits; the call's kernels are %.2f x this)" % (u, gbs(out_bytes, u), K, k / u))
        say("    today: to the host and numpy %8.1f ms %8.3f GB/s of elements   (host wall, one run over %.1f MiB of %d segments)"
            % (today, gbs(took, today), took / MIB, upto))
        say("    equal to the reference: %s" % ("no segment short enough to compare" if not checked else "yes" if same else "NO"))
        del dst, copy_dst, sum_dst, fields, src
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
