#!/usr/bin/env python3
"""The unnull kernels (csrc/brotli_unnull_kernels.hip) against the ragged copy and against what a caller does without them, for DESIGN section 8:

    python tools/unnull_bench.py [--out FILE] [--runs 7] [--shapes pages,one] [--widths 4,8] [--nulls 1,30,90] [--patterns scattered,runs]

Per case -- definition levels of one bit in device memory, and the dense values of the rows that are there --, four measurements, taken IN TURNS
(run r of each before run r + 1 of any) in one process, the median of --runs runs after two warm-up runs of each, with the spread (min .. max):
  (a) unnull   BrotliAmdBatchUnnullSegments with capacities from a counting call: the four launches' milliseconds together
               (BrotliAmdBatchLastUnnullMs: HIP events around them) and each phase's share (1: the walk, 2: the counts, 3: the carries, 4: the
               expansion);
  (b) copy     the same DESTINATION bytes moved device to device: the ragged copy's hook (BrotliAmdDebugRaggedCopy, host wall: it allocates and
               uploads its table as well) and one contiguous copy of as many bytes between HIP events; the SMALLER of the two;
  (c) today    what a caller has without these calls: BrotliAmdBatchUnrleSegments into one-byte levels (BrotliAmdBatchLastUnrleMs), then, between
               HIP events, torch's compare with the level, the spreading -- the FASTER of masked_scatter_ into zeros and cumsum, gather and where --
               and the bitmap's pack by bit weights; the sum;
  (d) host     a device-to-host copy plus the numpy reference (tests/null_ref.py), host wall, ONE run over at most --host-mib MiB of destination.
The shapes: `pages`, 256 pages of 2^20 rows (sixteen different ones), and `one`, one segment of 2^26 rows; slots of 4 and 8 bytes; about 1, 30 and
90 % nulls, SCATTERED -- every row drawn by itself, so the levels are bit-packed runs of 504 --, and in RUNS -- stretches of 8 .. 2000 rows of
one kind, so they are RLE runs.
TWO BOUNDS.  (a) <= (c) + (c)'s own run-to-run spread (max - min) in this session: (c) is the code callers would otherwise keep.  (a) as a
multiple of (b), beside the floor that the bytes alone give: (b) moves m w bytes each way, (a) reads the levels and V w and writes m w + m / 8;
nothing is gated on that ratio, the excess is attributed per phase.  The first run's results, slots and bitmaps are compared with (c)'s, and the
first segment's with the reference.  Exit status 1 where a comparison or the first bound fails."""
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
import null_ref as ref  # noqa: E402
import rle_ref  # noqa: E402

MIB = 1 << 20
SHAPES = {"pages": (256, 1 << 20, 16), "one": (1, 1 << 26, 1)}   # segments, rows a segment, different segments


def levels_scattered(rng, rows, null_pct):
    """every row drawn by itself: bit-packed runs of 504 levels (63 groups, the longest a one-byte header names) -> (bytes, the mask)"""
    assert rows % 504 == 0 or rows % 8 == 0
    mask = rng.random(rows) >= null_pct / 100.0
    packed = np.packbits(mask, bitorder="little")
    full = rows // 504
    body = np.empty((full, 64), dtype=np.uint8)
    body[:, 0] = 63 << 1 | 1
    body[:, 1:] = packed[:full * 63].reshape(full, 63)
    out = body.tobytes()
    rest = rows - full * 504
    if rest:
        out += rle_ref.header(rest // 8 << 1 | 1) + packed[full * 63:].tobytes()
    return out, mask


def levels_runs(rng, rows, null_pct):
    """stretches of 8 .. 2000 rows of one kind, nulls with their share of the rows: RLE runs -> (bytes, the mask)"""
    out, mask, at = [], np.zeros(rows, dtype=bool), 0
    while at < rows:
        n = min(int(rng.integers(8, 2001)), rows - at)
        there = rng.random() >= null_pct / 100.0
        out.append(rle_ref.header(n << 1) + bytes([1 if there else 0]))
        mask[at:at + n] = there
        at += n
    return b"".join(out), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--shapes", default="pages,one")
    ap.add_argument("--widths", default="4,8")
    ap.add_argument("--nulls", default="1,30,90")
    ap.add_argument("--patterns", default="scattered,runs")
    ap.add_argument("--host-mib", type=int, default=16)
    a = ap.parse_args()
    shapes, widths, nulls, patterns = a.shapes.split(","), [int(w) for w in a.widths.split(",")], [int(p) for p in a.nulls.split(",")], a.patterns.split(",")
    if a.runs < 1 or any(s not in SHAPES for s in shapes) or any(w not in (1, 2, 4, 8) for w in widths) or any(p not in ("scattered", "runs") for p in patterns):
        ap.error("--runs: at least 1; --shapes: of pages,one; --widths: of 1,2,4,8; --patterns: of scattered,runs")
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

    def timed(fn):
        """fn() between two HIP events on the current stream -> milliseconds"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    say("library %s; item %d slots, walk chunk %d bytes, carry span %d items" % (os.environ.get("BROTLI_AMD_LIB", "(the tree's)"), pkg.unrle_item_elems(), pkg.unrle_walk_chunk(),
                                                                                  pkg.undelta_carry_span()))
    ok = True
    for shape in shapes:
        n, rows, distinct = SHAPES[shape]
        for pattern in patterns:
            for pct in nulls:
                rng = np.random.default_rng(20310 + pct)
                kinds = [(levels_scattered if pattern == "scattered" else levels_runs)(rng, rows, pct) for _ in range(distinct)]
                offs, lens, at = [], [], 0
                for i in range(n):
                    offs.append(at); lens.append(len(kinds[i % distinct][0]))
                    at += lens[-1]
                host = np.zeros(at + 16, dtype=np.uint8)
                for i in range(n):
                    host[offs[i]:offs[i] + lens[i]] = np.frombuffer(kinds[i % distinct][0], dtype=np.uint8)
                src = torch.from_numpy(host).cuda()
                present = [int(kinds[i % distinct][1].sum()) for i in range(n)]
                total, V = n * rows, sum(present)
                for W in widths:
                    dtype = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[W]
                    values = torch.randint(1, 256, (max(V * W, 8),), dtype=torch.uint8, device="cuda")   # (never 0: a slot that is there shows)
                    dst = torch.empty(total * W + 128, dtype=torch.uint8, device="cuda")
                    copy_dst = torch.empty(total * W + 128, dtype=torch.uint8, device="cuda")
                    valid = torch.empty(total // 8 + 128, dtype=torch.uint8, device="cuda")
                    lv = torch.empty(total, dtype=torch.uint8, device="cuda")
                    two_dst = torch.empty(total, dtype=dtype, device="cuda")
                    two_valid = torch.empty(total // 8, dtype=torch.uint8, device="cuda")
                    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
                    typed = values.view(dtype)
                    zero = torch.zeros((), dtype=dtype, device="cuda")
                    sync()
                    sp, vp, dp, bp, lp = src.data_ptr(), values.data_ptr(), dst.data_ptr(), valid.data_ptr(), lv.data_ptr()
                    v_offs = np.concatenate([[0], np.cumsum(present)[:-1]]).astype(np.int64) * W
                    a_src = (ctypes.c_void_p * n)(*[sp + o for o in offs])
                    a_len = (ctypes.c_size_t * n)(*lens)
                    a_val = (ctypes.c_void_p * n)(*[vp + int(o) for o in v_offs])
                    a_cnt = (ctypes.c_uint64 * n)(*present)
                    a_dst = (ctypes.c_void_p * n)(*[dp + i * rows * W for i in range(n)])
                    a_bit = (ctypes.c_void_p * n)(*[bp + i * rows // 8 for i in range(n)])
                    a_ldst = (ctypes.c_void_p * n)(*[lp + i * rows for i in range(n)])
                    a_cap = (ctypes.c_uint64 * n)(*([rows] * n))
                    a_k = (ctypes.c_uint8 * n)(*([1] * n))
                    a_level = (ctypes.c_uint32 * n)(*([1] * n))
                    a_w = (ctypes.c_uint8 * n)(*([W] * n))
                    a_w1 = (ctypes.c_uint8 * n)(*([1] * n))
                    a_cdst = (ctypes.c_void_p * n)(*[copy_dst.data_ptr() + i * rows * W for i in range(n)])
                    a_clen = (ctypes.c_size_t * n)(*([rows * W] * n))
                    res = (pkg.UnnullResult * n)()
                    res_rle = (pkg.UnrleResult * n)()

                    def unnull():
                        if L.BrotliAmdBatchUnnullSegments(batch._h, n, a_src, a_len, a_val, a_cnt, a_dst, a_bit, a_cap, a_k, a_level, a_w, None, res, None) != 0:
                            raise RuntimeError(pkg.last_error())
                        return batch.last_unnull_ms(), [batch.last_unnull_ms(p) for p in (1, 2, 3, 4)]

                    def unrle():
                        if L.BrotliAmdBatchUnrleSegments(batch._h, n, a_src, a_len, a_ldst, a_cap, a_k, a_w1, None, res_rle, None) != 0:
                            raise RuntimeError(pkg.last_error())
                        return batch.last_unrle_ms()

                    def copy():
                        t0 = time.perf_counter()
                        if L.BrotliAmdDebugRaggedCopy(n, a_dst, a_cdst, a_clen) != 0:
                            raise RuntimeError(pkg.last_error())
                        hook = (time.perf_counter() - t0) * 1e3
                        return min(hook, timed(lambda: copy_dst[:total * W].copy_(dst[:total * W])))

                    def pack(mask):
                        torch.sum(mask.view(-1, 8).to(torch.uint8) * weights, dim=1, dtype=torch.uint8, out=two_valid)

                    def spread_scatter():
                        mask = lv == 1
                        two_dst.zero_()
                        two_dst.masked_scatter_(mask, typed)
                        pack(mask)

                    def spread_ranks():
                        mask = lv == 1
                        ranks = torch.cumsum(mask, 0) - 1
                        torch.where(mask, typed[ranks.clamp_(min=0, max=max(V - 1, 0))] if V else zero, zero, out=two_dst)
                        pack(mask)

                    t = {key: [] for key in ("unnull", "p1", "p2", "p3", "p4", "unrle", "copy", "scatter", "ranks")}
                    same = True
                    for run in range(-2, a.runs):
                        sync()
                        u, ph = unnull()
                        r = unrle()
                        c = copy()
                        s1 = timed(spread_scatter)
                        s2 = timed(spread_ranks)
                        if run == -2:   # against what the caller's steps give, and the first segment against the reference
                            same = torch.equal(two_dst.view(torch.uint8), dst[:total * W]) and torch.equal(two_valid, valid[:total // 8])
                            same = same and all(res[i].astuple() == (rows, lens[i], res[i].runs, 0, 1, present[i], 0, present[i]) for i in range(n))
                            if rows <= 1 << 20:
                                slots, bits, want = ref.outputs(kinds[0][0], 1, 1, W, 0, values[:present[0] * W].cpu().numpy().tobytes(), present[0], rows)
                                same = same and dst[:rows * W].cpu().numpy().tobytes() == slots and valid[:rows // 8].cpu().numpy().tobytes() == bits and res[0].astuple() == want
                            ok = ok and same
                        if run >= 0:
                            for key, v in zip(t, (u, ph[0], ph[1], ph[2], ph[3], r, c, s1, s2)):
                                t[key].append(v)
                    # (d): the bytes to the host, and the reference over them
                    upto = max(1, min(n, a.host_mib * MIB // (rows * W)))
                    part = min(rows, a.host_mib * MIB // W)   # (of one long segment: its first rows)
                    t0 = time.perf_counter()
                    back = src[:offs[upto - 1] + lens[upto - 1]].cpu().numpy()
                    back_values = values[:sum(present[:upto]) * W].cpu().numpy().tobytes()
                    v_at = 0
                    for i in range(upto):
                        ref.decode(back[offs[i]:offs[i] + lens[i]].tobytes(), 1, 1, W, 0, back_values[v_at:], present[i], part)
                        v_at += present[i] * W
                    host_ms = (time.perf_counter() - t0) * 1e3
                    med = {key: statistics.median(v) for key, v in t.items()}
                    best = "scatter" if med["scatter"] <= med["ranks"] else "ranks"
                    today = [x + y for x, y in zip(t["unrle"], t[best])]
                    span = lambda v: "%.3f .. %.3f" % (min(v), max(v))   # noqa: E731
                    u, c, td = med["unnull"], med["copy"], statistics.median(today)
                    spread = max(today) - min(today)
                    level_bytes = sum(lens)
                    floor = (level_bytes + V * W + total * W + total / 8) / (2.0 * total * W)
                    say("%s, %s, %d %% nulls, %d-byte slots (%d segments, %d rows, %d there, %.1f MiB of levels, %.1f MiB of slots; median of %d, min .. max)"
                        % (shape, pattern, pct, W, n, total, V, level_bytes / MIB, total * W / MIB, a.runs))
                    say("    (a) unnull, four launches   %9.3f ms (%s) %8.1f GB/s of slots   (phases 1 / 2 / 3 / 4: %.3f / %.3f / %.3f / %.3f ms = %.0f / %.0f / %.0f / %.0f %%)"
                        % (u, span(t["unnull"]), total * W / u / 1e6, med["p1"], med["p2"], med["p3"], med["p4"], 100 * med["p1"] / u, 100 * med["p2"] / u, 100 * med["p3"] / u,
                           100 * med["p4"] / u))
                    say("    (b) copy of the slots' bytes %8.3f ms (%s)   (a) is %.2f x this; the bytes alone give %.2f x" % (c, span(t["copy"]), u / c, floor))
                    say("    (c) unrle into levels       %9.3f ms (%s); masked_scatter_ and pack %.3f ms (%s); cumsum, gather, where and pack %.3f ms (%s)"
                        % (med["unrle"], span(t["unrle"]), med["scatter"], span(t["scatter"]), med["ranks"], span(t["ranks"])))
                    say("    (c) today: unrle + %-8s %9.3f ms (%s)   (a) is %.2f x this" % (best, td, span(today), u / td))
                    say("    (d) to the host and numpy   %9.1f ms %8.3f GB/s of slots   (host wall, one run over %d segments, %d rows each)"
                        % (host_ms, upto * part * W / host_ms / 1e6, upto, part))
                    say("    equal to the caller's steps and the reference: %s" % ("yes" if same else "NO"))
                    met = u <= td + spread
                    ok = ok and met
                    say("    BOUND (a) <= (c) + (c)'s spread: %s (%.3f ms against %.3f + %.3f ms)" % ("met" if met else "MISSED", u, td, spread))
                    del dst, copy_dst, valid, lv, two_dst, two_valid, values, typed
                del src
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
