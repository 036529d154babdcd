#!/usr/bin/env python3
"""The undict kernels (csrc/brotli_undict_kernels.hip) against unrle, against the ragged copy and against what a caller does without them, for
DESIGN section 8:

    python tools/undict_bench.py [--out FILE] [--runs 10] [--legs a,b,c,d]

Per leg of segments in device memory -- dictionary-index runs of Parquet's RLE / bit-packed hybrid --, five measurements, taken IN TURNS (run r
of each before run r + 1 of any) in one process, the median of --runs runs after two warm-up runs of each, with the spread (min .. max):
  undict    BrotliAmdBatchUndictSegments with capacities from a counting call: the two launches' milliseconds together
            (BrotliAmdBatchLastUndictMs: HIP events around them) and each phase's share (1: the walk, 2: the expansion with the lookup);
  unrle     BrotliAmdBatchUnrleSegments over the same segments into 4-byte indices (BrotliAmdBatchLastUnrleMs);
  copy      the same DESTINATION bytes moved device to device: the ragged copy's hook (BrotliAmdDebugRaggedCopy, host wall: it allocates and
            uploads its table as well) and one contiguous copy of as many bytes between HIP events; the SMALLER of the two is what the bound
            takes;
  two-step  what a caller has today: that unrle call, then torch indexing of the concatenated dictionaries by the concatenated indices (rebased
            per dictionary where a leg has several), between HIP events; the sum of the two;
  today     a device-to-host copy plus the numpy reference (tests/dict_ref.py), host wall, ONE run over at most --today-mib MiB of destination.
The legs: (a) 1024 pages of 64 Ki values, 12-bit indices, a dictionary of 4096 x 4 bytes per page group (sixteen groups), runs of 8 .. 504
packed and 8 .. 2000 repeated values; (b) the same pages with 8-byte values and ONE dictionary of 2^20 entries under uniformly random 20-bit
indices -- the gather's worst case: 8 MiB --, and (b') the same with the indices kept below 4096, which says what of (b) the fetched dictionary
explains; (c) long repeated runs only (1000 .. 60 000 values); (d) 100 000 segments of 40 values at mixed alignments.
TWO BOUNDS are checked on (a) and (c), where the dictionary stays in cache: undict <= unrle + copy -- no two-step can beat that sum, since it
writes the indices and then writes the values --, and undict <= the measured two-step.  (b) and (d) are recorded without a gate.  The first
run's results and the elements of the first segments are compared with the reference.  Exit status 1 where a comparison or a bound fails."""
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
import dict_ref as ref  # noqa: E402
import rle_ref  # noqa: E402

MIB = 1 << 20


def segment(rng, k, values, packed, repeated, below):
    """seeded runs that hold at least `values` values of k bits below `below`: packed ones of packed[0] .. packed[1] values (None: none),
    repeated ones of repeated[0] .. repeated[1] (None: none) -> bytes"""
    out, have = [], 0
    while have < values:
        if repeated is None or (packed is not None and rng.integers(2)):
            g = int(rng.integers(packed[0] // 8, packed[1] // 8 + 1))
            if below == 1 << k:   # every field seeded bits
                payload = rng.integers(0, 256, size=g * k, dtype=np.uint8).tobytes()
            else:
                payload = rle_ref.pack_fields([int(v) for v in rng.integers(0, below, size=8 * g)], k)
            out.append(rle_ref.header(g << 1 | 1) + payload)
            have += 8 * g
        else:
            c = int(rng.integers(repeated[0], repeated[1] + 1))
            out.append(rle_ref.header(c << 1) + int(rng.integers(0, below)).to_bytes((k + 7) // 8, "little"))
            have += c
    return b"".join(out)


LEGS = {   # name -> (title, segments, values a segment, distinct segments, k, w, entries, dictionaries, indices below, packed, repeated, mixed, gated)
    "a": ("(a) 1024 pages of 64 Ki values, 12-bit indices, 4096 x 4 bytes a page group", 1024, 1 << 16, 16, 12, 4, 4096, 16, 4096, (8, 504), (8, 2000), False, True),
    "b": ("(b) the same pages, 8-byte values, ONE dictionary of 2^20 entries, random 20-bit indices", 1024, 1 << 16, 16, 20, 8, 1 << 20, 1, 1 << 20, (8, 504), (8, 2000), False, False),
    "b'": ("(b') as (b), the indices below 4096", 1024, 1 << 16, 16, 20, 8, 1 << 20, 1, 4096, (8, 504), (8, 2000), False, False),
    "c": ("(c) long repeated runs only: 1024 pages of 64 Ki values, runs of 1000 .. 60 000", 1024, 1 << 16, 16, 12, 4, 4096, 16, 4096, None, (1000, 60000), False, True),
    "d": ("(d) 100 000 segments of 40 values at mixed alignments", 100000, 40, 64, 12, 4, 4096, 1, 4096, (8, 16), (1, 12), True, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--legs", default="a,b,b',c,d")
    ap.add_argument("--today-mib", type=int, default=16)
    a = ap.parse_args()
    names = a.legs.split(",")
    if a.runs < 1 or any(name not in LEGS for name in names):
        ap.error("--runs: at least 1; --legs: of " + ",".join(LEGS))
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

    say("library %s; item %d elements, walk chunk %d bytes" % (os.environ.get("BROTLI_AMD_LIB", "(the tree's)"), pkg.unrle_item_elems(), pkg.unrle_walk_chunk()))
    ok = True
    for name in names:
        title, n, values, distinct, K, W, D, ndict, below, packed, repeated, mixed, gated = LEGS[name]
        rng = np.random.default_rng(20290)
        kinds = [segment(rng, K, values, packed, repeated, below) for _ in range(distinct)]
        offs, lens, at = [], [], 0
        for i in range(n):
            at += i % 5 if mixed else 0
            offs.append(at); lens.append(len(kinds[i % distinct]))
            at += lens[-1]
        host = np.zeros(at + 16, dtype=np.uint8)
        for i in range(n):
            host[offs[i]:offs[i] + lens[i]] = np.frombuffer(kinds[i % distinct], dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        table = rng.integers(0, 256, size=ndict * D * W, dtype=np.uint8)
        d_table = torch.from_numpy(table).cuda()
        sync()
        sp, tp = src.data_ptr(), d_table.data_ptr()
        which = [i % distinct % ndict for i in range(n)]   # a segment's dictionary: its page group's
        counted = batch.undict_segments([sp + o for o in offs], lens, None, [0] * n, [K] * n, [W] * n, None, None, None)
        total, runs = sum(r[0] for r in counted), sum(r[2] for r in counted)
        say("%s (%d segments, %.1f MiB of source, %d values in %d runs, %.1f MiB of values, %d dictionar%s of %.2f MiB; median of %d, min .. max)"
            % (title, n, sum(lens) / MIB, total, runs, total * W / MIB, ndict, "y" if ndict == 1 else "ies", D * W / MIB, a.runs))
        if any(r[3] != ref.OK for r in counted):
            say("  a segment did not end well: %r" % ([r for r in counted if r[3] != ref.OK][:3],))
            ok = False
            continue
        d_offs, i_offs, at, i_at = [], [], 0, 0
        for i, r in enumerate(counted):
            at += i % 7 if mixed else 0
            d_offs.append(at); i_offs.append(i_at)
            at += r[0] * W; i_at += r[0] * 4
        out_bytes = total * W
        dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty(at + 128, dtype=torch.uint8, device="cuda")
        idx = torch.empty(total, dtype=torch.int32, device="cuda")   # the two-step's indices, back to back and aligned
        typed = d_table.view({4: torch.int32, 8: torch.int64}[W])
        base = None
        if ndict > 1:   # the rebase per dictionary: every element's dictionary's first entry
            base = torch.repeat_interleave(torch.tensor([w * D for w in which], dtype=torch.int32, device="cuda"),
                                           torch.tensor([r[0] for r in counted], device="cuda"))
        two_dst = torch.empty(total, dtype=typed.dtype, device="cuda")
        dp, ip = dst.data_ptr(), idx.data_ptr()
        a_src = (ctypes.c_void_p * n)(*[sp + o for o in offs])
        a_len = (ctypes.c_size_t * n)(*lens)
        a_dst = (ctypes.c_void_p * n)(*[dp + o for o in d_offs])
        a_idst = (ctypes.c_void_p * n)(*[ip + o for o in i_offs])
        a_cap = (ctypes.c_uint64 * n)(*[r[0] for r in counted])
        a_k = (ctypes.c_uint8 * n)(*([K] * n))
        a_w = (ctypes.c_uint8 * n)(*([W] * n))
        a_w4 = (ctypes.c_uint8 * n)(*([4] * n))
        a_dict = (ctypes.c_void_p * n)(*[tp + w * D * W for w in which])
        a_D = (ctypes.c_uint64 * n)(*([D] * n))
        a_cdst = (ctypes.c_void_p * n)(*[copy_dst.data_ptr() + o for o in d_offs])
        a_clen = (ctypes.c_size_t * n)(*[r[0] * W for r in counted])
        res = (pkg.UndictResult * n)()
        res_rle = (pkg.UnrleResult * n)()

        def undict():
            if L.BrotliAmdBatchUndictSegments(batch._h, n, a_src, a_len, a_dst, a_cap, a_k, a_w, None, a_dict, a_D, res, None) != 0:
                raise RuntimeError(pkg.last_error())
            return batch.last_undict_ms(), [batch.last_undict_ms(p) for p in (1, 2)]

        def unrle():
            if L.BrotliAmdBatchUnrleSegments(batch._h, n, a_src, a_len, a_idst, a_cap, a_k, a_w4, None, res_rle, None) != 0:
                raise RuntimeError(pkg.last_error())
            return batch.last_unrle_ms()

        def copy():
            t0 = time.perf_counter()
            if L.BrotliAmdDebugRaggedCopy(n, a_dst, a_cdst, a_clen) != 0:
                raise RuntimeError(pkg.last_error())
            hook = (time.perf_counter() - t0) * 1e3
            return min(hook, timed(lambda: copy_dst[:out_bytes].copy_(dst[:out_bytes])))

        def gather():
            if base is None:
                return timed(lambda: torch.index_select(typed, 0, idx, out=two_dst))
            return timed(lambda: torch.index_select(typed, 0, idx + base, out=two_dst))

        t = {key: [] for key in ("undict", "p1", "p2", "unrle", "copy", "gather")}
        same, checked = True, 0
        for run in range(-2, a.runs):
            sync()
            u, ph = undict()
            r = unrle()
            c = copy()
            g = gather()
            if run == -2:   # the first segments against the reference, and the two-step against undict
                for i in range(min(n, 24)):
                    part = table[which[i] * D * W:(which[i] + 1) * D * W].tobytes()
                    elems, want = ref.elements_bytes(kinds[i % distinct], K, W, 0, part, D, counted[i][0])
                    got = dst[d_offs[i]:d_offs[i] + counted[i][0] * W].cpu().numpy().tobytes()
                    same = same and got == elems and res[i].astuple() == want
                    checked += 1
                if not mixed:
                    same = same and torch.equal(two_dst.view(torch.uint8), dst[:out_bytes])
                ok = ok and same
            if run >= 0:
                for key, v in zip(("undict", "p1", "p2", "unrle", "copy", "gather"), (u, ph[0], ph[1], r, c, g)):
                    t[key].append(v)
        # today: the bytes to the host, and the reference over them
        upto, took = 0, 0
        for i in range(n):
            if took + counted[i][0] * W > a.today_mib * MIB and took:
                break
            upto += 1; took += counted[i][0] * W
        t0 = time.perf_counter()
        back = src[:offs[upto - 1] + lens[upto - 1]].cpu().numpy()
        back_table = d_table.cpu().numpy()
        for i in range(upto):
            ref.decode(back[offs[i]:offs[i] + lens[i]].tobytes(), K, W, 0, back_table[which[i] * D * W:(which[i] + 1) * D * W].tobytes(), D)
        today = (time.perf_counter() - t0) * 1e3
        med = {key: statistics.median(v) for key, v in t.items()}
        two = [x + y for x, y in zip(t["unrle"], t["gather"])]
        both = [x + y for x, y in zip(t["unrle"], t["copy"])]
        span = lambda v: "%.3f .. %.3f" % (min(v), max(v))   # noqa: E731
        gbs = lambda b, ms: b / ms / 1e6   # noqa: E731
        u = med["undict"]
        say("    undict, two launches        %9.3f ms (%s) %8.1f GB/s of values   (phases 1 / 2: %.3f / %.3f ms = %.0f / %.0f %%)"
            % (u, span(t["undict"]), gbs(out_bytes, u), med["p1"], med["p2"], 100 * med["p1"] / u, 100 * med["p2"] / u))
        say("    unrle into 4-byte indices   %9.3f ms (%s)" % (med["unrle"], span(t["unrle"])))
        say("    copy of the values' bytes   %9.3f ms (%s)" % (med["copy"], span(t["copy"])))
        say("    unrle + copy                %9.3f ms (%s)   undict is %.2f x this" % (statistics.median(both), span(both), u / statistics.median(both)))
        say("    torch indexing by the indices %7.3f ms (%s)" % (med["gather"], span(t["gather"])))
        say("    two-step: unrle + indexing  %9.3f ms (%s)   undict is %.2f x this" % (statistics.median(two), span(two), u / statistics.median(two)))
        say("    today: to the host and numpy %8.1f ms %8.3f GB/s of values   (host wall, one run over %.1f MiB of %d segments)"
            % (today, gbs(took, today), took / MIB, upto))
        say("    equal to the reference: %s" % ("yes" if same else "NO"))
        if gated:
            for what, bound in (("unrle + copy", statistics.median(both)), ("the two-step", statistics.median(two))):
                met = u <= bound
                ok = ok and met
                say("    BOUND undict <= %s: %s (%.3f ms against %.3f ms)" % (what, "met" if met else "MISSED", u, bound))
        del dst, copy_dst, idx, two_dst, src, d_table, base
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
