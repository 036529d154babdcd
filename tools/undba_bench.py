#!/usr/bin/env python3
"""The undba kernels (csrc/brotli_undba_kernels.hip) against the route a caller has today and against undlba on the same strings, for DESIGN
section 8:

    python tools/undba_bench.py [--out FILE] [--runs 5] [--mib 64]

Per row -- DELTA_BYTE_ARRAY page bodies of sorted strings of about L bytes of which a share of 0, 50 or 90 % is the prefix they have in common
with the string in front, as MANY SMALL PAGES of 4097 values each (at most 256 of them, about --mib MiB of strings) and as ONE LARGE PAGE (half
of --mib MiB of strings, 8192 .. 262144 values) --, measurements taken IN TURNS (run r of each before
run r + 1 of any) in one process, the median of --runs runs after two warm-up runs of each, with the spread (min .. max):
  fused     BrotliAmdBatchUndbaSegments with capacities from a measuring call: the nine launches' milliseconds together
            (BrotliAmdBatchLastUndbaMs: HIP events around them), each phase's share (BrotliAmdBatchLastUndbaPhaseMs 1..9), and the call's host
            wall;
  today     the route a caller has without the call: BrotliAmdBatchUndbpSegments over the prefix lengths, `consumed` read on the host, the same
            over the suffix lengths, then both arrays of lengths and the suffix bytes copied to the host, and there the prefix chain, page by
            page; host wall of all of it.  The host's chain is pyarrow's reader where pyarrow imports -- pq.read_table over one in-memory file
            of the same column written with DELTA_BYTE_ARRAY, which decodes the lengths once more: said here, not hidden -- and its version is
            printed; the chain alone in plain Python over one page is printed beside it;
  undlba    BrotliAmdBatchUndlbaSegments over the SAME strings written as DELTA_LENGTH_BYTE_ARRAY: what is left of `fused` above it is the
            price of the prefix phases.
Nothing is gated: the table says where the fused call loses.  The first run's offsets and bytes are compared with the strings.  Exit status 1
where that comparison fails."""
import argparse
import io
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
import dba_ref as ref  # noqa: E402
import dlba_ref  # noqa: E402


def strings_of(rnd, values, L, share):
    """sorted strings of L bytes: the first share x L bytes come from a slowly changing stem, the rest are seeded"""
    stem_len = L * share // 100
    out, stem = [], bytearray(rnd.randbytes(stem_len))
    for i in range(values):
        if stem_len and i % 8 == 0:
            stem[rnd.randrange(stem_len // 2, stem_len)] = rnd.randrange(256)
        out.append(bytes(stem) + rnd.randbytes(L - stem_len))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--lengths", default="16,1024")
    ap.add_argument("--shares", default="0,50,90")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        pa = pq = None
    pkg = load_pkg()
    sync = torch.cuda.synchronize
    batch = pkg.Batch(1)

    def say(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def wall(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    spread = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))   # noqa: E731
    say("item %d deltas; median of %d runs (min .. max), milliseconds; host decode: %s" %
        (pkg.undbp_item_deltas(), a.runs, "pyarrow %s, pq.read_table of an in-memory file" % pa.__version__ if pa else "no pyarrow: the plain Python chain alone"))
    ok = True
    for L in [int(x) for x in a.lengths.split(",")]:
        for share in [int(x) for x in a.shares.split(",")]:
            for shape, n, values in (("many small pages", max(2, min(256, (a.mib << 20) // (4097 * L))), 4097), ("one large page", 1, max(8192, min(262144, (a.mib << 19) // L)))):
                rnd = random.Random(L * 1000 + share)
                strings = strings_of(rnd, values, L, share)
                body, plain = ref.encode(strings), dlba_ref.encode(strings)
                total = sum(len(s) for s in strings)
                step = (max(len(body), len(plain)) + 63) & ~63
                up = lambda raw: torch.from_numpy(np.frombuffer(raw + bytes(step - len(raw)), dtype=np.uint8).copy()).cuda().repeat(n)   # noqa: E731
                src, src_l = up(body), up(plain)
                o_step, d_step = (4 * (values + 1) + 63) & ~63, (total + 63) & ~63
                d_o, d_d = torch.empty(n * o_step + 64, dtype=torch.uint8, device="cuda"), torch.empty(n * d_step + 64, dtype=torch.uint8, device="cuda")
                t_p, t_s = torch.empty(n * o_step // 4 + 16, dtype=torch.int32, device="cuda"), torch.empty(n * o_step // 4 + 16, dtype=torch.int32, device="cuda")
                sync()
                srcs, srcs_l = [src.data_ptr() + i * step for i in range(n)], [src_l.data_ptr() + i * step for i in range(n)]
                o_ptrs, d_ptrs = [d_o.data_ptr() + i * o_step for i in range(n)], [d_d.data_ptr() + i * d_step for i in range(n)]
                measured = batch.undba_segments(srcs, [len(body)] * n, None, None, None, [values] * n)
                if any(m[ref.R_BYTES] != total or m[ref.R_STATUS] != 0 for m in measured):
                    say("  a page did not measure well: %r" % (measured[:1],))
                    ok = False
                    continue
                table = None
                if pa:
                    buf = io.BytesIO()
                    pq.write_table(pa.table([pa.array(strings, type=pa.binary())], schema=pa.schema([pa.field("c", pa.binary(), nullable=False)])), buf, use_dictionary=False,
                                   column_encoding={"c": "DELTA_BYTE_ARRAY"}, compression="NONE", write_statistics=False, data_page_size=1 << 30)
                    table = buf.getvalue()

                def fused():
                    t0 = time.perf_counter()
                    res = batch.undba_segments(srcs, [len(body)] * n, o_ptrs, d_ptrs, [total] * n, [values] * n)
                    return batch.last_undba_ms(), [batch.last_undba_ms(p) for p in range(1, 10)], (time.perf_counter() - t0) * 1e3, res

                def today():
                    def work():
                        res = batch.undbp_segments(srcs, [len(body)] * n, [t_p.data_ptr() + i * o_step for i in range(n)], [values] * n, [4] * n)
                        ms = batch.last_undbp_ms()
                        at = [r[1] for r in res]   # (on the host: where the suffix lengths begin)
                        res = batch.undbp_segments([s + c for s, c in zip(srcs, at)], [len(body) - c for c in at], [t_s.data_ptr() + i * o_step for i in range(n)], [values] * n, [4] * n)
                        ms += batch.last_undbp_ms()
                        p_host, s_host, bytes_host = t_p.cpu(), t_s.cpu(), src.cpu()
                        if table is not None:
                            for _ in range(n):
                                pq.read_table(io.BytesIO(table))
                        return ms, (p_host, s_host, bytes_host)
                    return wall(work)

                def undlba():
                    batch.undlba_segments(srcs_l, [len(plain)] * n, o_ptrs, d_ptrs, [total] * n, [values] * n)
                    return batch.last_undlba_ms()

                t = {key: [] for key in ("fused", "wall", "today", "undbp", "undlba")}
                phases = [[] for _ in range(9)]
                same = True
                for run in range(-2, a.runs):
                    sync()
                    f, ph, w, res = fused()
                    if run == -2:
                        got_o = d_o[:4 * (values + 1)].view(torch.int32).cpu().tolist()
                        same = got_o == ref.column(body)[0] and d_d[:total].cpu().numpy().tobytes() == b"".join(strings)
                        same = same and torch.equal(d_d[(n - 1) * d_step:(n - 1) * d_step + total], d_d[:total])
                        ok = ok and same
                    td, (ub, _) = today()
                    ul = undlba()
                    if run >= 0:
                        for key, v in zip(t, (f, w, td, ub, ul)):
                            t[key].append(v)
                        for p in range(9):
                            phases[p].append(ph[p])
                # the chain alone in plain Python, one page
                t0 = time.perf_counter()
                ref.column(body)
                chain = (time.perf_counter() - t0) * 1e3
                f = statistics.median(t["fused"])
                say("L %d, %d %% shared, %s: %d page%s of %d values, %.1f MiB of strings" % (L, share, shape, n, "" if n == 1 else "s", values, n * total / (1 << 20)))
                say("    fused, nine launches    %-30s %7.2f GB/s of strings   phases 1..9 %%: %s; host wall %s" %
                    (spread(t["fused"]), n * total / f / 1e6, " / ".join("%.0f" % (100 * statistics.median(p) / f) for p in phases), spread(t["wall"])))
                say("    its phases A, B, C      %s / %s / %s" % (spread(phases[6]), spread(phases[7]), spread(phases[8])))
                say("    today's route           %-30s (host wall; the two undbp calls' kernels in it %s)   fused wall / today %.3f" %
                    (spread(t["today"]), spread(t["undbp"]), statistics.median(t["wall"]) / statistics.median(t["today"])))
                say("    undlba, same strings    %-30s fused / undlba %.2f" % (spread(t["undlba"]), f / statistics.median(t["undlba"])))
                say("    the reference's chain over one page in plain Python: %.1f ms; equal to the strings: %s" % (chain, "yes" if same else "NO"))
                del src, src_l, d_o, d_d, t_p, t_s
    batch.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
