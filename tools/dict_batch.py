#!/usr/bin/env python3
"""What a shared custom dictionary gives a batch of small documents: 64 unique documents of 8 KiB that share
one 64 KiB dictionary, each emitted twice with tools/brotli_emit.py -- against the dictionary and self-contained -- and each set
repeated to 4096 streams.  Both batches are decoded with decode_device + relaunch, inputs resident, warmed up; the kernel time
is BrotliAmdBatchLastKernelMs.  Reports compressed bytes, ms and GB/s of output for both.

    python tools/dict_batch.py [--streams 4096] [--steps 5] [--out profiles/dict_batch.txt]

The self-contained batch run on another build of the library (BROTLI_AMD_LIB=<that library>: one without the dictionary entry
points skips the dictionary batch) is the baseline for time."""
import argparse
import importlib.util
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def load_pkg():
    import torch
    torch.cuda.init()   # (torch's copy of the HIP runtime first: tests/conftest.py)
    name = "rust_brotli_decompressor_amd"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def documents(n_unique=64, doc_bytes=8192, dict_bytes=65536, seed=2026):
    import dict_gen as ds
    rnd = random.Random(seed)
    D = ds.text(rnd, dict_bytes, "etaoinshrdlucmfwyp", 4000)
    docs = [ds.related(rnd, D, doc_bytes, fresh=0.35) for _ in range(n_unique)]
    with_dict = [ds.stream_for(d, 18, D) for d in docs]   # (stream_for checks the emitter's own data; run() checks what the device decodes)
    alone = [ds.stream_for(d, 18, b"") for d in docs]
    return D, docs, with_dict, alone


def run(pkg, torch, comps, docs, dictionary, n_streams, steps):
    dev = torch.device("cuda:0")
    t_in = [torch.frombuffer(bytearray(c), dtype=torch.uint8).to(dev) for c in comps]
    t_dict = torch.frombuffer(bytearray(dictionary), dtype=torch.uint8).to(dev) if dictionary else None
    cap = max(len(d) for d in docs)
    out = torch.zeros(n_streams * cap, dtype=torch.uint8, device=dev)
    k = len(comps)
    in_ptrs = [t_in[i % k].data_ptr() for i in range(n_streams)]
    in_sizes = [len(comps[i % k]) for i in range(n_streams)]
    out_ptrs = [out.data_ptr() + i * cap for i in range(n_streams)]
    caps = [len(docs[i % k]) for i in range(n_streams)]
    torch.cuda.synchronize()
    batch = pkg.Batch(n_streams)
    kw = {}
    if t_dict is not None:
        kw = dict(dict_ptrs=[t_dict.data_ptr()] * n_streams, dict_sizes=[len(dictionary)] * n_streams)
    batch.decode_device(in_ptrs, in_sizes, out_ptrs, caps, 1, None, **kw)
    res = batch.wait()
    assert all(r.result == 1 and r.decoded_size == c for r, c in zip(res, caps)), [(r.result, r.error_code) for r in res[:4]]
    for i in (0, k - 1, n_streams - 1):
        assert bytes(out[i * cap:i * cap + caps[i]].cpu().numpy()) == docs[i % k]
    ms = []
    for _ in range(1 + steps):   # (the first relaunch: warm-up)
        batch.relaunch(); batch.wait(); ms.append(batch.last_kernel_ms())
    batch.close()
    ms = sorted(ms[1:])
    return sum(in_sizes), sum(caps), ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_pkg()
    import torch
    D, docs, with_dict, alone = documents()
    lines = ["dict_batch: %d streams (64 unique documents of %d bytes), one shared dictionary of %d bytes; device %s; library %s"
             % (a.streams, len(docs[0]), len(D), torch.cuda.get_device_name(0), os.path.basename(os.path.dirname(pkg.LIB_PATH)) + "/" + os.path.basename(pkg.LIB_PATH))]
    legs = [("self-contained", alone, None)]
    if hasattr(pkg.load_library(), "BrotliAmdBatchDecodeDeviceDict"):
        legs.append(("shared dictionary", with_dict, D))
    for label, comps, d in legs:
        cbytes, obytes, med, lo, hi = run(pkg, torch, comps, docs, d, a.streams, a.steps)
        lines.append("%-18s compressed %9d bytes  output %9d bytes  kernel %.3f ms (min %.3f, max %.3f, %d steps)  %.2f GB/s of output"
                     % (label, cbytes, obytes, med, lo, hi, a.steps, obytes / med / 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
