#!/usr/bin/env python3
"""The undict-bytes kernels (csrc/brotli_undict_bytes_kernels.hip) against the ragged copy's floor, against undict over the same index runs and
against what a caller has without them, for DESIGN section 8:

    python tools/undict_bytes_bench.py [--out FILE] [--runs 5] [--mib 64]

Per row -- pages of dictionary-index runs over ONE dictionary of D byte arrays whose lengths are uniform in [L / 2, 3 L / 2], about --mib MiB of
strings in all --, four measurements, taken IN TURNS (run r of each before run r + 1 of any) in one process, the median of --runs runs after two
warm-up runs of each, with the spread (min .. max):
  fused     BrotliAmdBatchUndictBytesSegments with data capacities from a measuring call: the five launches' milliseconds together
            (BrotliAmdBatchLastUndictBytesMs: HIP events around them) and each phase's share (1: the dictionary walk, 2: the RLE walk, 3: the
            lengths, 4: the carries, 5: the expansion); the dictionary walk's time per entry beside it;
  floor     the same data bytes plus the offsets' bytes moved device to device, one contiguous copy between HIP events;
  undict    BrotliAmdBatchUndictSegments at w = 8 over the same index runs and a dictionary of D x 8 bytes: what the shared phases -- the walk,
            the indices, a lookup an element -- cost (BrotliAmdBatchLastUndictMs);
  torch     the route a caller has without the fused call: BrotliAmdBatchUnrleSegments into an int32 index tensor (BrotliAmdBatchLastUnrleMs),
            then torch on the device -- the lengths indexed, a cumsum, and a repeat_interleave-and-gather for the bytes, with the dictionary's
            starts made on the host (not timed) --, between HIP events; the sum of the two.
Rows: L of 4, 16, 64 and 1024, D of 16, 4096 and 65536, runs that are RLE-heavy (repeats of 100 .. 2000, packed runs of 8 .. 16) and
bit-packed-heavy (packed runs of 8 .. 504 only).  Nothing is gated: the table says where the fused call does not beat the torch route.  The
first run's offsets and bytes are compared with the torch route's.  Exit status 1 where that comparison fails."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stream_sessions import load_pkg  # noqa: E402
from undict_bench import segment  # noqa: E402

MIB = 1 << 20
KINDS = {"rle-heavy": ((8, 16), (100, 2000)), "packed-heavy": ((8, 504), None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--lengths", default="4,16,64,1024")
    ap.add_argument("--entries", default="16,4096,65536")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    pkg = load_pkg()
    sync = torch.cuda.synchronize
    batch = pkg.Batch(1)

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    say("item %d elements, walk chunk %d bytes; about %d MiB of strings a row; median of %d runs (min .. max), milliseconds" % (pkg.unrle_item_elems(), pkg.unrle_walk_chunk(), a.mib, a.runs))
    say("%5s %6s %-12s | %8s %-17s %-29s %9s | %8s | %8s | %8s = %6s + %7s | %s" % ("L", "D", "runs", "fused", "(min .. max)", "phases 1/2/3/4/5 %", "walk/entry", "floor", "undict8",
                                                                                   "torch", "unrle", "torch", "fused / torch"))
    ok = True
    for L in [int(x) for x in a.lengths.split(",")]:
        for D in [int(x) for x in a.entries.split(",")]:
            for kind, (packed, repeated) in KINDS.items():
                rng = np.random.default_rng(20291)
                K = max(1, (D - 1).bit_length())
                values = max(1024, min(65536, a.mib * MIB // (256 * L)))
                n = max(1, a.mib * MIB // (values * L))
                lens = rng.integers(L // 2, 3 * L // 2 + 1, size=D).astype(np.int64)
                starts = np.cumsum(lens + 4) - lens   # the position of every entry's first value byte
                blob = rng.integers(1, 256, size=int(starts[-1] + lens[-1]), dtype=np.uint8)
                for e in range(D):
                    blob[starts[e] - 4:starts[e]] = np.frombuffer(int(lens[e]).to_bytes(4, "little"), dtype=np.uint8)
                kinds = [segment(rng, K, values, packed, repeated, D) for _ in range(16)]
                offs, slens, at = [], [], 0
                for i in range(n):
                    offs.append(at); slens.append(len(kinds[i % 16])); at += slens[-1]
                host = np.zeros(at + 16, dtype=np.uint8)
                for i in range(n):
                    host[offs[i]:offs[i] + slens[i]] = np.frombuffer(kinds[i % 16], dtype=np.uint8)
                src, d_blob = torch.from_numpy(host).cuda(), torch.from_numpy(blob).cuda()
                d8 = torch.from_numpy(rng.integers(0, 256, size=D * 8, dtype=np.uint8)).cuda()
                t_lens, t_starts = torch.from_numpy(lens).cuda(), torch.from_numpy(starts).cuda()
                sync()
                sp, tp = src.data_ptr(), d_blob.data_ptr()
                srcs = [sp + o for o in offs]
                counted = batch.undict_bytes_segments(srcs, slens, None, None, None, [0] * n, [K] * n, None, None, None, None)   # (the rows: a page header's)
                measured = batch.undict_bytes_segments(srcs, slens, None, None, None, [r[0] for r in counted], [K] * n, None, None, [tp] * n, [len(blob)] * n, [D] * n)
                if any(r[3] != 0 or r[5] != 0 or r[10] != 0 for r in measured):
                    say("  a segment did not end well: %r" % ([r for r in measured if r[3] or r[5] or r[10]][:2],))
                    ok = False
                    continue
                counts, nbytes = [r[0] for r in measured], [r[7] for r in measured]
                total, total_bytes = sum(counts), sum(nbytes)
                o_offs, d_offs, o_at, d_at = [], [], 0, 0
                for c, b in zip(counts, nbytes):   # one Arrow array a page, each at a multiple of 64 bytes
                    o_offs.append(o_at); d_offs.append(d_at)
                    o_at += (4 * (c + 1) + 63) & ~63; d_at += (b + 63) & ~63
                d_o, d_d = torch.empty(o_at + 64, dtype=torch.uint8, device="cuda"), torch.empty(d_at + 64, dtype=torch.uint8, device="cuda")
                c_o, c_d = torch.empty_like(d_o), torch.empty_like(d_d)
                idx, vals8 = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int64, device="cuda")
                i_offs = [4 * sum(counts[:i]) for i in range(n)] if n < 4096 else list(np.cumsum([0] + [4 * c for c in counts[:-1]]))
                op, dp, ip, vp = d_o.data_ptr(), d_d.data_ptr(), idx.data_ptr(), vals8.data_ptr()

                def fused():
                    batch.undict_bytes_segments(srcs, slens, [op + o for o in o_offs], [dp + o for o in d_offs], nbytes, counts, [K] * n, None, None, [tp] * n, [len(blob)] * n, [D] * n)
                    return batch.last_undict_bytes_ms(), [batch.last_undict_bytes_ms(p) for p in (1, 2, 3, 4, 5)]

                def floor():
                    return timed(lambda: (c_o.copy_(d_o), c_d.copy_(d_d)))

                def undict8():
                    batch.undict_segments(srcs, slens, [vp + 2 * o for o in i_offs], counts, [K] * n, [8] * n, None, [d8.data_ptr()] * n, [D] * n)
                    return batch.last_undict_ms()

                route = {}

                def torch_route():
                    batch.unrle_segments(srcs, slens, [ip + o for o in i_offs], counts, [K] * n, [4] * n)
                    rle = batch.last_unrle_ms()

                    def work():
                        i64 = idx.long()
                        ls = t_lens[i64]
                        ends = torch.cumsum(ls, 0)
                        first = ends - ls
                        where = torch.repeat_interleave(t_starts[i64] - first, ls) + torch.arange(int(total_bytes), device="cuda")
                        route["ends"], route["data"] = ends, d_blob[where]
                    return rle, timed(work)

                t = {key: [] for key in ("fused", "p1", "p2", "p3", "p4", "p5", "floor", "undict8", "rle", "torch")}
                same = True
                for run in range(-2, a.runs):
                    sync()
                    f, ph = fused()
                    c = floor()
                    u = undict8()
                    r, g = torch_route()
                    if run == -2:   # the fused call's pages, one behind the other, are the torch route's one array
                        got_d = torch.cat([d_d[o:o + b] for o, b in zip(d_offs, nbytes)])
                        got_o = torch.cat([d_o[o:o + 4 * (c_ + 1)].view(torch.int32)[1:].long() + base for o, c_, base in zip(o_offs, counts, np.cumsum([0] + nbytes[:-1]).tolist())])
                        same = torch.equal(got_d, route["data"]) and torch.equal(got_o, route["ends"])
                        ok = ok and same
                    if run >= 0:
                        for key, v in zip(t, (f, *ph, c, u, r, g)):
                            t[key].append(v)
                med = {key: statistics.median(v) for key, v in t.items()}
                both = [x + y for x, y in zip(t["rle"], t["torch"])]
                f = med["fused"]
                say("%5d %6d %-12s | %8.3f %-17s %-29s %7.1f ns | %8.3f | %8.3f | %8.3f = %6.3f + %7.3f | %.2f%s" %
                    (L, D, kind, f, "(%.3f .. %.3f)" % (min(t["fused"]), max(t["fused"])), " / ".join("%.0f" % (100 * med[p] / f) for p in ("p1", "p2", "p3", "p4", "p5")),
                     1e6 * med["p1"] / D, med["floor"], med["undict8"], statistics.median(both), med["rle"], med["torch"], f / statistics.median(both),
                     "" if same else "   NOT EQUAL to the torch route"))
                del src, d_blob, d_o, d_d, c_o, c_d, idx, vals8, route
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
