#!/usr/bin/env python3
"""The undlba kernels (csrc/brotli_undlba_kernels.hip) against the ragged copy, against the route a caller had with undbp alone and against the
host, for DESIGN section 8:

    python tools/undlba_bench.py [--out FILE] [--runs 5] [--mib 64] [--lengths 4,16,64,1024]

Per row -- DELTA_LENGTH_BYTE_ARRAY page bodies of strings whose lengths are uniform in [L / 2, 3 L / 2], about --mib MiB of strings in all, as
MANY SMALL PAGES of 4097 values each and as ONE LARGE PAGE of as many values --, four measurements, taken IN TURNS (run r of each before run
r + 1 of any) in one process, the median of --runs runs after two warm-up runs of each, with the spread (min .. max):
  fused     BrotliAmdBatchUndlbaSegments with capacities and data capacities from a counting call: the seven launches' milliseconds together
            (BrotliAmdBatchLastUndlbaMs: HIP events around them) and each phase's share (1: the walk, 2: the delta sums, 3: their carries, 4:
            the lengths, 5: their carries, 6: the offsets, 7: the data), and the call's host wall;
  copy      the ragged copy kernel moving the same data AND offset bytes device to device, a segment a page and destination
            (BrotliAmdDebugRaggedCopy: its whole hook as host wall), and one contiguous device-to-device copy of as many bytes between HIP
            events;
  today     the route a caller has without the call: BrotliAmdBatchUndbpSegments into int32 lengths (its kernels: BrotliAmdBatchLastUndbpMs),
            then per page a torch.cumsum over an element-aligned view, `consumed` read from the results on the host, and a copy of the page's
            bytes; host wall of all of it, waited for;
  host      a device-to-host copy of the pages plus the numpy reference (tests/dlba_ref.py) over at most --today-mib MiB of them, host wall.
Nothing is gated: the table says where the fused call does not beat today's route.  The first run's offsets and bytes are compared with
today's route's.  Exit status 1 where that comparison fails."""
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
import dbp_ref  # noqa: E402
import dlba_ref as ref  # noqa: E402

MIB = 1 << 20
PATTERN = 4096   # deltas of the pattern that a page repeats: 32 blocks of 128


def pattern(rng, L):
    """-> (the blocks of PATTERN deltas that lead from a length back to itself, that length, the lengths behind each delta)"""
    lens = rng.integers(L // 2, 3 * L // 2 + 1, size=PATTERN).astype(np.int64)
    stream = dbp_ref.encode([int(v) for v in lens] + [int(lens[0])])
    header = len(dbp_ref.varint(128) + dbp_ref.varint(4) + dbp_ref.varint(PATTERN + 1) + dbp_ref.varint(dbp_ref.zigzag(int(lens[0]))))
    return stream[header:], int(lens[0]), np.concatenate([lens[1:], lens[:1]])


def page(blocks, first, repeats):
    """the lengths' stream of a page of repeats x PATTERN + 1 values"""
    return dbp_ref.varint(128) + dbp_ref.varint(4) + dbp_ref.varint(repeats * PATTERN + 1) + dbp_ref.varint(dbp_ref.zigzag(first)) + blocks * repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--lengths", default="4,16,64,1024")
    ap.add_argument("--today-mib", type=int, default=8)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    pkg = load_pkg()
    sync = torch.cuda.synchronize
    batch, lib = pkg.Batch(1), pkg.load_library()

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    spread = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))   # noqa: E731
    say("item %d deltas; about %d MiB of strings a row; median of %d runs (min .. max), milliseconds" % (pkg.undbp_item_deltas(), a.mib, a.runs))
    ok = True
    for L in [int(x) for x in a.lengths.split(",")]:
        rng = np.random.default_rng(20311 + L)
        blocks, first, lens = pattern(rng, L)
        per = int(lens.sum())   # bytes of one repeat
        repeats = max(1, a.mib * MIB // per)
        for shape, n, r in (("many small pages", repeats, 1), ("one large page", 1, repeats)):
            body_lengths = page(blocks, first, r)
            values, nbytes = r * PATTERN + 1, first + r * per
            step = (len(body_lengths) + nbytes + 63) & ~63
            one = np.zeros(step, dtype=np.uint8)
            one[:len(body_lengths)] = np.frombuffer(body_lengths, dtype=np.uint8)
            one[len(body_lengths):len(body_lengths) + nbytes] = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
            src = torch.from_numpy(one).cuda().repeat(n)   # (every page the same bytes: nothing here depends on them)
            sync()
            sp = src.data_ptr()
            srcs, slens = [sp + i * step for i in range(n)], [len(body_lengths) + nbytes] * n
            counted = batch.undlba_segments(srcs, slens, None, None, None, [0] * n)
            if any(c[4] != 0 or c[0] != values or c[11] != nbytes for c in counted):
                say("  a page did not count well: %r" % (counted[:2],))
                ok = False
                continue
            o_step, d_step = (4 * (values + 1) + 63) & ~63, (nbytes + 63) & ~63
            d_o, d_d = torch.empty(n * o_step + 64, dtype=torch.uint8, device="cuda"), torch.empty(n * d_step + 64, dtype=torch.uint8, device="cuda")
            c_o, c_d = torch.empty_like(d_o), torch.empty_like(d_d)
            t_l = torch.empty(n * o_step // 4 + 16, dtype=torch.int32, device="cuda")    # today's lengths, a page at a multiple of 64 bytes
            t_o, t_d = torch.zeros_like(d_o), torch.empty_like(d_d)
            op, dp = d_o.data_ptr(), d_d.data_ptr()
            o_ptrs, d_ptrs = [op + i * o_step for i in range(n)], [dp + i * d_step for i in range(n)]
            copy_src = (ctypes.c_void_p * (2 * n))(*(o_ptrs + d_ptrs))
            copy_dst = (ctypes.c_void_p * (2 * n))(*([c_o.data_ptr() + i * o_step for i in range(n)] + [c_d.data_ptr() + i * d_step for i in range(n)]))
            copy_len = (ctypes.c_size_t * (2 * n))(*([4 * (values + 1)] * n + [nbytes] * n))
            moved = n * (4 * (values + 1) + nbytes)

            def fused():
                t0 = time.perf_counter()
                res = batch.undlba_segments(srcs, slens, o_ptrs, d_ptrs, [nbytes] * n, [values] * n)
                return batch.last_undlba_ms(), [batch.last_undlba_ms(p) for p in range(1, 8)], (time.perf_counter() - t0) * 1e3, res

            def copies():
                w, rc = wall(lambda: lib.BrotliAmdDebugRaggedCopy(2 * n, copy_src, copy_dst, copy_len))
                if rc != 0:
                    raise RuntimeError(pkg.last_error())
                return w, timed(lambda: (c_o.copy_(d_o), c_d.copy_(d_d)))

            def today():
                def work():
                    res = batch.undbp_segments(srcs, slens, [t_l.data_ptr() + i * o_step for i in range(n)], [values] * n, [4] * n)
                    for i in range(n):
                        consumed = res[i][1]   # (on the host: the call has waited and brought the results)
                        ends = t_o[i * o_step + 4:i * o_step + 4 * (values + 1)].view(torch.int32)
                        torch.cumsum(t_l[i * o_step // 4:i * o_step // 4 + values], 0, dtype=torch.int32, out=ends)
                        t_d[i * d_step:i * d_step + nbytes].copy_(src[i * step + consumed:i * step + consumed + nbytes])
                    return batch.last_undbp_ms()
                return wall(work)

            t = {key: [] for key in ("fused", "wall", "ragged", "floor", "today", "undbp")}
            phases = [[] for _ in range(7)]
            same = True
            for run in range(-2, a.runs):
                sync()
                f, ph, w, res = fused()
                rc, fl = copies()
                td, ub = today()
                if run == -2:
                    same = all(x[7] == 0 and x[8] == 0 and x[10] == nbytes for x in res)
                    for i in range(min(n, 64)):   # the first pages, whole
                        same = same and torch.equal(d_o[i * o_step:i * o_step + 4 * (values + 1)], t_o[i * o_step:i * o_step + 4 * (values + 1)])
                        same = same and torch.equal(d_d[i * d_step:i * d_step + nbytes], t_d[i * d_step:i * d_step + nbytes])
                    ok = ok and same
                if run >= 0:
                    for key, v in zip(t, (f, w, rc, fl, td, ub)):
                        t[key].append(v)
                    for p in range(7):
                        phases[p].append(ph[p])
            # the host: the pages back, and the reference over them
            upto = min(n, a.today_mib * MIB // slens[0])
            host = None
            if upto:
                t0 = time.perf_counter()
                back = src[:upto * step].cpu().numpy()
                for i in range(upto):
                    ref.column(back[i * step:i * step + slens[i]].tobytes(), values)
                host = (time.perf_counter() - t0) * 1e3
            f, td = statistics.median(t["fused"]), statistics.median(t["today"])
            gbs = lambda ms: moved / ms / 1e6   # noqa: E731
            say("L %d, %s: %d page%s of %d values, %.1f MiB of strings, %.1f MiB of offsets" % (L, shape, n, "" if n == 1 else "s", values, n * nbytes / MIB, n * 4 * (values + 1) / MIB))
            say("    fused, seven launches   %-30s %7.1f GB/s   phases 1..7 %%: %s; host wall %s" %
                (spread(t["fused"]), gbs(f), " / ".join("%.0f" % (100 * statistics.median(p) / f) for p in phases), spread(t["wall"])))
            say("    its data phase alone    %-30s" % spread(phases[6]))
            say("    ragged copy, same bytes %-30s (its hook, host wall); one contiguous copy %s (events)" % (spread(t["ragged"]), spread(t["floor"])))
            say("    today's route           %-30s (host wall; undbp's kernels in it %s)   fused wall / today %.2f" % (spread(t["today"]), spread(t["undbp"]), statistics.median(t["wall"]) / td))
            say("    host: copy back + numpy %s" % ("%.1f ms over %d page%s (host wall, one run)" % (host, upto, "" if upto == 1 else "s") if host is not None else "not run: one page is above --today-mib"))
            say("    equal to today's route: %s" % ("yes" if same else "NO"))
            del src, d_o, d_d, c_o, c_d, t_l, t_o, t_d
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
