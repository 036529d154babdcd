#!/usr/bin/env python3
"""N open streaming sessions, each handed CHUNK bytes of its .br stream a round -- the proxy's, the server's, the loader's view of the
streaming ABI -- once as a loop of BrotliDecoderDecompressStream calls, state by state, and once through a stream set
(include/brotli/batch.h: BrotliAmdStreamSetDecompress), which steps all of them with one launch.

    python tools/stream_sessions.py N CHUNK [--out FILE] [--mode both|solo|set] [--repeat R]

The streams are the golden fixtures of a few KiB to a few hundred KiB compressed and, where an encoder library is there, two of
workloads.py's generators; session i gets stream i modulo their number.  A round gives every session that is not done its next CHUNK bytes
and room for all the output it has; a session that wants more room is called again with no input.  Printed per mode and repeat: the rounds,
wall milliseconds in all and per round, decode launches and host <-> device copies of payload per round (the set counts its own:
BrotliAmdStreamSetLastLaunches / LastTransfers; a solo call that decodes is one launch and two copies), and whether every session's bytes
hash to what the stream decodes to.  --repeat alternates the modes R times (same process, same device: the comparison the numbers are for).
A library without stream sets (an older build, through BROTLI_AMD_LIB) runs the solo loop alone."""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURES = ["alice29.txt.compressed", "lcet10.txt.compressed", "plrabn12.txt.compressed", "mapsdatazrh.compressed",
            "compressed_repeated.compressed", "random_org_10k.bin.compressed", "asyoulik.txt.compressed", "monkey.compressed"]


def load_pkg():
    try:   # (torch brings its own HIP runtime: where it is used in the process at all, it has to come first)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    spec = importlib.util.spec_from_file_location("rust_brotli_decompressor_amd", os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rust_brotli_decompressor_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def streams():
    """-> [(name, compressed, sha256 of the decoded bytes)]"""
    import workloads as w
    gold = os.path.join(ROOT, "tests", "golden")
    manifest = {e["name"]: e for e in json.load(open(os.path.join(gold, "manifest.json")))}
    out = []
    for name in FIXTURES:
        path = os.path.join(gold, "testdata", name)
        if os.path.exists(path) and name in manifest:
            out.append((name, open(path, "rb").read(), manifest[name]["sha256"]))
    if w.encoder_available():
        for kind, gen in (("long_backref 512 KiB", w.long_backref_stream), ("high_entropy 128 KiB", w.high_entropy_stream)):
            raw = gen(7, (512 << 10) if kind.startswith("long") else (128 << 10))
            out.append((kind, w.brotli_compress(raw, 5, 22), hashlib.sha256(raw).hexdigest()))
    return out


def run(pkg, mode, sessions, chunk):
    """-> dict of the run's figures"""
    L = pkg.load_library()
    n = len(sessions)
    states = [pkg.DecoderState(large_window=True) for _ in range(n)]
    sset = pkg.StreamSet(n) if mode == "set" else None
    cap = max(1 << 16, 8 * chunk)
    src = [ctypes.create_string_buffer(c, max(1, len(c))) for _, c, _ in sessions]
    outb = [ctypes.create_string_buffer(cap) for _ in range(n)]
    base, oaddr = [ctypes.addressof(b) for b in src], [ctypes.addressof(b) for b in outb]
    st = (ctypes.c_void_p * n)(*[s._h for s in states])
    ai, ao, ni, no, tot = ((ctypes.c_size_t * n)() for _ in range(5))
    res = (ctypes.c_int * n)()
    solo = L["BrotliDecoderDecompressStream"]
    solo.argtypes = [ctypes.c_void_p] * 6
    A = [ctypes.addressof(a) for a in (ai, ni, ao, no, tot)]
    size = [len(c) for _, c, _ in sessions]
    pos, hashes, done = [0] * n, [hashlib.sha256() for _ in range(n)], [False] * n
    more_room = [False] * n   # the last call wanted more output room: called again without new input
    live = list(range(n))
    rounds = launches = transfers = 0
    t0 = time.perf_counter()
    while live:
        for i in live:
            give = 0 if more_room[i] else min(chunk, size[i] - pos[i])
            ai[i] = give; ni[i] = base[i] + pos[i]; ao[i] = cap; no[i] = oaddr[i]
        if sset is not None:
            for i in range(n):
                if done[i]:
                    ai[i] = 0; ao[i] = cap; no[i] = oaddr[i]
            if L.BrotliAmdStreamSetDecompress(sset._h, n, st, ai, ni, ao, no, tot, res) != 0:
                raise RuntimeError(pkg.last_error())
            launches += sset.last_launches(); transfers += sset.last_transfers()
        else:
            for i in live:
                if ai[i]:
                    launches += 1; transfers += 2   # (its chunk in, its output back; a call whose output buffer had to grow launches again)
                o = 8 * i
                res[i] = solo(st[i], A[0] + o, A[1] + o, A[2] + o, A[3] + o, A[4] + o)
        nxt = []
        for i in live:
            give = 0 if more_room[i] else min(chunk, size[i] - pos[i])
            pos[i] += give - ai[i]
            made = cap - ao[i]
            if made:
                hashes[i].update(ctypes.string_at(oaddr[i], made))
            r = res[i]
            more_room[i] = r == 3
            if r in (0, 1) or (r == 2 and pos[i] >= size[i]):
                done[i] = True
            else:
                nxt.append(i)
        live = nxt
        rounds += 1
    wall = (time.perf_counter() - t0) * 1e3
    ok = all(res[i] == 1 and hashes[i].hexdigest() == sessions[i][2] for i in range(n))
    if sset is not None:
        sset.close()
    for s in states:
        s.close()
    return dict(mode=mode, sessions=n, chunk=chunk, rounds=rounds, wall_ms=round(wall, 3), ms_per_round=round(wall / max(1, rounds), 4),
                launches_per_round=round(launches / max(1, rounds), 2), transfers_per_round=round(transfers / max(1, rounds), 2), ok=ok)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n", type=int)
    ap.add_argument("chunk", type=int)
    ap.add_argument("--out")
    ap.add_argument("--mode", default="both", choices=["both", "solo", "set"])
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    pkg = load_pkg()
    have_sets = hasattr(pkg.load_library(), "BrotliAmdStreamSetDecompress") and hasattr(pkg, "StreamSet")
    modes = ["solo", "set"] if a.mode == "both" else [a.mode]
    if not have_sets:
        modes = [m for m in modes if m == "solo"]
    pool = streams()
    sessions = [pool[i % len(pool)] for i in range(a.n)]
    run(pkg, modes[0], sessions[: min(a.n, 8)], a.chunk)   # (the first launches of a process pay for the device's start: not the figures')
    lines = []
    for rep in range(a.repeat):
        for m in modes:
            r = run(pkg, m, sessions, a.chunk)
            r["repeat"] = rep
            r["library"] = os.path.basename(os.path.dirname(pkg.LIB_PATH)) + "/" + os.path.basename(pkg.LIB_PATH)
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(l)["ok"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
