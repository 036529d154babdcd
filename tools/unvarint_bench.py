#!/usr/bin/env python3
"""The unvarint kernels (csrc/brotli_unvarint_kernels.hip) against the ragged copy, against undelta's read-only pass and against what a caller
does without them, for DESIGN section 8:

    python tools/unvarint_bench.py [--out FILE] [--runs 10] [--rows metric,one64,one1g,small,tiny] [--mixes ones,proto,fives,tens] [--widths 4,8]

Per row of segments in device memory, per mix of varint lengths and per element width, four legs, taken IN TURNS (run k of each before run
k + 1 of any), the median of --runs runs after two warm-up runs of each:
  unvarint  BrotliAmdBatchUnvarintSegments with capacities from a counting call: the three launches' milliseconds together
            (BrotliAmdBatchLastUnvarintMs: HIP events around them), each phase's share of them (1: the tiles' counts, 2: the carries, 3: the
            elements), GB/s of SOURCE bytes and of DESTINATION bytes over them, and the whole call as host wall time (table upload, launches,
            wait, results);
  copy      the ragged copy kernel moving the same DESTINATION bytes device to device (BrotliAmdDebugRaggedCopy: its whole hook as host wall
            time, which allocates and uploads its table as well): what writing that many bytes costs;
  read      undelta's phase 1 over the same SOURCE bytes at width 1 (BrotliAmdBatchLastUndeltaPhaseMs(1) of a BrotliAmdBatchUndeltaSegments
            call): the read-only pass this kernel also makes;
  today     a device-to-host copy of the source and the numpy reference (tests/varint_ref.py) over it, as host wall time, ONE run, over at
            most the first --today-mib MiB of the row's segments (the rate is what is compared).
The mixes: "ones" all 1-byte varints, "proto" 70 / 25 / 5 % of 1 / 2 / 3-5 bytes, "fives" all 5 bytes, "tens" all 10 bytes.  A segment cuts the
varints where it begins and ends, so a row of many segments has unfinished bytes at its edges.
The first run's results and elements of the first segments are compared with the reference."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stream_sessions import load_pkg  # noqa: E402
import varint_ref as ref  # noqa: E402

MIB = 1 << 20
MIXES = {"ones": "all 1-byte", "proto": "70 / 25 / 5 % of 1 / 2 / 3-5 bytes", "fives": "all 5-byte", "tens": "all 10-byte"}


def rows():
    """name -> (title, [(offset, length)]): segments of one source buffer (the sets of tools/undelta_bench.py)"""
    rnd = random.Random(8)
    tiny, at = [], 0
    for _ in range(100000):
        at += rnd.randrange(0, 16)
        tiny.append((at, 100)); at += 100
    return {
        "metric": ("256 x 4 MiB of source", [(i * 4 * MIB, 4 * MIB) for i in range(256)]),
        "one64": ("one segment of 64 MiB", [(0, 64 * MIB)]),
        "one1g": ("one segment of 1 GiB", [(0, 1024 * MIB)]),
        "small": ("small documents: 4096 x 8 KiB", [(i * 8192, 8192) for i in range(4096)]),
        "tiny": ("tiny segments: 100 000 x 100 B at mixed alignments", tiny),
    }


def varint_bytes(mix, size, seed):
    """`size` bytes of varints of the mix's lengths, random bits in them: 16 MiB of them, over and over"""
    if size > 16 * MIB:
        return np.resize(varint_bytes(mix, 16 * MIB, seed), size)
    rng = np.random.default_rng(seed)
    if mix == "ones":
        return rng.integers(0, 0x80, size=size, dtype=np.uint8)
    n = size   # (more varints than fit: the bytes are cut at `size`)
    if mix == "proto":
        lens = rng.choice(np.array([1, 2, 3, 4, 5]), size=n // 2 + 16, p=[0.70, 0.25, 0.05 / 3, 0.05 / 3, 0.05 / 3])
    else:
        lens = np.full(n // (5 if mix == "fives" else 10) + 16, 5 if mix == "fives" else 10)
    ends = np.cumsum(lens) - 1
    ends = ends[ends < size]
    a = rng.integers(0, 0x100, size=size, dtype=np.uint8) | 0x80
    a[ends] &= 0x7F
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", default="metric,one64,one1g,small,tiny")
    ap.add_argument("--mixes", default="ones,proto,fives,tens")
    ap.add_argument("--widths", default="4,8")
    ap.add_argument("--today-mib", type=int, default=16)
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs: at least 1")
    table = rows()
    names, mixes = a.rows.split(","), a.mixes.split(",")
    for name in names:
        if name not in table:
            ap.error("--rows: one of " + ",".join(table))
    for mix in mixes:
        if mix not in MIXES:
            ap.error("--mixes: one of " + ",".join(MIXES))
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
    src = torch.empty(room + 128, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(room + 128, dtype=torch.uint8, device="cuda")   # where undelta's pass writes
    assert src.data_ptr() % 64 == 0
    batch = pkg.Batch(1)

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    say("tile %d bytes of source, carry span %d tiles" % (pkg.unvarint_tile(), pkg.undelta_carry_span()))
    ok = True
    for mix in mixes:
        host = varint_bytes(mix, room, 20276)
        src[:room].copy_(torch.from_numpy(host))
        sync()
        for name in names:
            title, segs = table[name]
            n, nbytes = len(segs), sum(l for _, l in segs)
            sp = src.data_ptr()
            a_src = (ctypes.c_void_p * n)(*[sp + o for o, _ in segs])
            a_len = (ctypes.c_size_t * n)(*[l for _, l in segs])
            counted = batch.unvarint_segments([sp + o for o, _ in segs], [l for _, l in segs], None, [0] * n, [1] * n)
            count_ms = batch.last_unvarint_ms()
            total = sum(c for c, _, _ in counted)
            say("%s; %s (%d segments, %.1f MiB, %d varints, %d overlong; counting alone %.3f ms; median of %d)"
                % (title, MIXES[mix], n, nbytes / MIB, total, sum(v for _, _, v in counted), count_ms, a.runs))
            for w in widths:
                # destinations back to back, the tiny ones at mixed alignments
                offs, at = [], 0
                for i, (c, _, _) in enumerate(counted):
                    at += i % 7 if name == "tiny" else 0
                    offs.append(at)
                    at += c * w
                out_bytes = total * w
                dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
                copy_dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
                dp = dst.data_ptr()
                a_dst = (ctypes.c_void_p * n)(*[dp + o for o in offs])
                a_cap = (ctypes.c_uint64 * n)(*[c for c, _, _ in counted])
                a_w = (ctypes.c_uint8 * n)(*([w] * n))
                a_one = (ctypes.c_uint8 * n)(*([1] * n))
                a_scr = (ctypes.c_void_p * n)(*[scratch.data_ptr() + o for o, _ in segs])
                a_cdst = (ctypes.c_void_p * n)(*[copy_dst.data_ptr() + o for o in offs])
                a_clen = (ctypes.c_size_t * n)(*[c * w for c, _, _ in counted])
                res = (pkg.UnvarintResult * n)()

                def unvarint():
                    t0 = time.perf_counter()
                    if L.BrotliAmdBatchUnvarintSegments(batch._h, n, a_src, a_len, a_dst, a_cap, a_w, None, res, None) != 0:
                        raise RuntimeError(pkg.last_error())
                    wall = (time.perf_counter() - t0) * 1e3
                    return batch.last_unvarint_ms(), wall, [batch.last_unvarint_ms(p) for p in (1, 2, 3)]

                def copy():
                    t0 = time.perf_counter()
                    if L.BrotliAmdDebugRaggedCopy(n, a_dst, a_cdst, a_clen) != 0:
                        raise RuntimeError(pkg.last_error())
                    return (time.perf_counter() - t0) * 1e3

                def read():
                    if L.BrotliAmdBatchUndeltaSegments(batch._h, n, a_src, a_scr, a_len, a_one, None) != 0:
                        raise RuntimeError(pkg.last_error())
                    return batch.last_undelta_ms(1)

                kernel_ms, call_ms, copy_ms, read_ms, phase_ms = [], [], [], [], [[], [], []]
                same, checked = True, 0
                for run in range(-2, a.runs):
                    sync()
                    k, wall, ph = unvarint()
                    c = copy()
                    r = read()
                    if run == -2:   # the first segments against the reference
                        for i in range(min(n, 3 if nbytes > 64 * MIB else 40)):
                            o, l = segs[i]
                            if l > 8 * MIB:
                                continue
                            elems, want = ref.elements_bytes(host[o:o + l], w, 0, counted[i][0])
                            got = dst[offs[i]:offs[i] + counted[i][0] * w].cpu().numpy().tobytes()
                            same = same and got == elems and res[i].astuple() == want == counted[i]
                            checked += 1
                        ok = ok and same
                    if run >= 0:
                        kernel_ms.append(k); call_ms.append(wall); copy_ms.append(c); read_ms.append(r)
                        for p in range(3):
                            phase_ms[p].append(ph[p])
                # today: the bytes to the host, and the reference over them
                upto, took = 0, 0
                for o, l in segs:
                    if took + l > a.today_mib * MIB and took:
                        break
                    upto += 1; took += l
                t0 = time.perf_counter()
                back = src[:room].cpu().numpy() if took == nbytes else src[:segs[upto - 1][0] + segs[upto - 1][1]].cpu().numpy()
                for o, l in segs[:upto]:
                    ref.unvarint(back[o:o + l], w, 0)
                today = (time.perf_counter() - t0) * 1e3
                k, wall, c, r = (statistics.median(v) for v in (kernel_ms, call_ms, copy_ms, read_ms))
                ph = [statistics.median(v) for v in phase_ms]
                gbs = lambda b, ms: b / ms / 1e6   # noqa: E731
                say("  width %d (%.1f MiB of elements)" % (w, out_bytes / MIB))
                say("    unvarint, three launches %10.3f ms %8.1f GB/s of source %8.1f GB/s of elements   (phases 1 / 2 / 3: %.3f / %.3f / %.3f ms = %.0f / %.0f / %.0f %%)"
                    % (k, gbs(nbytes, k), gbs(out_bytes, k), ph[0], ph[1], ph[2], 100 * ph[0] / k, 100 * ph[1] / k, 100 * ph[2] / k))
                say("    the call, host wall      %10.3f ms %8.1f GB/s of source" % (wall, gbs(nbytes, wall)))
                say("    ragged copy of the elements %7.3f ms %8.1f GB/s of elements   (its hook, host wall; phase 3 is %.2f x this)" % (c, gbs(out_bytes, c), ph[2] / c))
                say("    undelta's phase 1 over the source %.3f ms %8.1f GB/s of source   (phase 1 is %.2f x this)" % (r, gbs(nbytes, r), ph[0] / r))
                say("    today: to the host and numpy %8.1f ms %8.3f GB/s of source   (host wall, one run over %.1f MiB of %d segments)"
                    % (today, gbs(took, today), took / MIB, upto))
                say("    equal to the reference: %s" % ("no segment short enough to compare" if not checked else "yes" if same else "NO"))
                del dst, copy_dst
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
