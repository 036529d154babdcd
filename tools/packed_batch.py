#!/usr/bin/env python3
"""What it costs a batch not to know its decoded sizes: one batch decoded two ways on the same device, in turns --
with the caller's capacities through decode_device + wait, and through the packed call (decode_device_packed: size walk, estimates,
growth, gather) -- inputs resident in device memory, the first turn of each a warm-up.  Per way: the decode kernels' time
(BrotliAmdBatchLastKernelMs: for the packed call all its decode launches), the call's wall time on the host, decode launches and
ragged-copy launches.  Two batches:

  documents   4096 x 8 KiB single-metablock documents (tools/dict_gen.py's generators, 64 distinct): every hint is exact
  metric      the benchmark's 256 x 4 MiB streams: several metablocks each, so estimates and growth

    python tools/packed_batch.py [--steps 5] [--unique 256] [--only documents|metric] [--out profiles/packed_batch.txt]
"""
import argparse
import hashlib
import importlib.util
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)


def load_pkg():
    import torch
    torch.cuda.init()   # (torch's copy of the HIP runtime first: tests/conftest.py)
    name = "rust_brotli_decompressor_amd"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def documents(n_unique=64, doc_bytes=8192, seed=2027):
    """-> [(compressed, raw size, sha256 of raw)]: self-contained single-metablock documents"""
    import dict_gen as ds
    rnd = random.Random(seed)
    D = ds.text(rnd, 65536, "etaoinshrdlucmfwyp", 4000)
    docs = [ds.related(rnd, D, doc_bytes, fresh=0.35) for _ in range(n_unique)]
    return [(ds.stream_for(d, 18, b""), len(d), hashlib.sha256(d).hexdigest()) for d in docs]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run(pkg, torch, unique, n, steps):
    dev = torch.device("cuda:0")
    t_in = [torch.frombuffer(bytearray(c), dtype=torch.uint8).to(dev) for c, _, _ in unique]
    k = len(unique)
    in_ptrs = [t_in[i % k].data_ptr() for i in range(n)]
    in_sizes = [len(unique[i % k][0]) for i in range(n)]
    caps = [unique[i % k][1] for i in range(n)]
    stride = (max(caps) + 255) // 256 * 256
    out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    out_ptrs = [out.data_ptr() + i * stride for i in range(n)]
    torch.cuda.synchronize()
    known, packed = pkg.Batch(n), pkg.Batch(n)
    rows = {"known": [], "packed": []}
    for step in range(1 + steps):
        t0 = time.perf_counter()
        known.decode_device(in_ptrs, in_sizes, out_ptrs, caps, 1, None)
        res = known.wait()
        wall = (time.perf_counter() - t0) * 1e3
        rows["known"].append((known.last_kernel_ms(), wall, 1, 0))
        t0 = time.perf_counter()
        pres, ptr, offsets = packed.decode_device_packed(in_ptrs, in_sizes, None, None, 0, 1)
        wall = (time.perf_counter() - t0) * 1e3
        rows["packed"].append((packed.last_kernel_ms(), wall, packed.last_packed_launches(), packed.last_packed_copies()))
        if step == 0:   # both ways decoded the batch, and the packed bytes are the streams' own
            assert all(r.result == 1 and r.decoded_size == c for r, c in zip(res, caps)), [(r.result, r.error_code) for r in res[:4]]
            assert all(r.result == 1 and r.decoded_size == c for r, c in zip(pres, caps)), [(r.result, r.error_code) for r in pres[:4]]
            assert offsets == [sum(caps[:i]) for i in range(n + 1)]
            blob = packed.packed_fetch(offsets[-1])
            for i in sorted({0, 1, k - 1, n // 2, n - 1}):
                assert hashlib.sha256(blob[offsets[i]:offsets[i + 1]]).hexdigest() == unique[i % k][2], i
            del blob
    known.close(); packed.close()
    stats = {}
    for way, r in rows.items():
        r = r[1:]
        stats[way] = (median([x[0] for x in r]), median([x[1] for x in r]), r[-1][2], r[-1][3])
    return sum(in_sizes), sum(caps), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--unique", type=int, default=256, help="distinct streams of the metric's batch")
    ap.add_argument("--only", choices=["documents", "metric"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_pkg()
    import torch
    lines = ["packed_batch: known capacities (decode_device + wait) against the packed call, in turns, median of %d steps; device %s"
             % (a.steps, torch.cuda.get_device_name(0))]
    legs = []
    if a.only in (None, "documents"):
        legs.append(("4096 x 8 KiB documents (64 distinct, one metablock each)", documents(), 4096))
    if a.only in (None, "metric"):
        import bench
        label, unique, n = bench.build_workload("longbackref_256x4MiB", a.unique)
        legs.append((label, unique, n))
    for label, unique, n in legs:
        cbytes, obytes, stats = run(pkg, torch, unique, n, a.steps)
        lines.append("%s: compressed %d bytes, output %d bytes" % (label, cbytes, obytes))
        for way in ("known", "packed"):
            kms, wall, launches, copies = stats[way]
            lines.append("  %-7s kernel %9.3f ms  wall %9.3f ms  launches %d  copies %d  %8.2f GB/s of output by wall time"
                         % (way, kms, wall, launches, copies, obytes / wall / 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
