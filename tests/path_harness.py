"""What the GPU tests of the hand-emitted stream families (test_gpu_words.py, test_gpu_copies.py, test_gpu_headers.py, test_gpu_literals.py,
test_gpu_dict_paths.py) and their loaders (word_vectors.py .. dict_vectors.py) share: the oracle comparison, the recipes of short / cut /
flipped copies, the constructor of a leg set, the legs -- one fresh process per command path of the device --, and the recurring test
bodies.  Each test file keeps its selection of vectors, its labels and what it asserts about its own family.

A stream of a set is (label, stream, capacity, flags, dictionary or None).  Run as a program -- path_harness.py MODULE SET -- this is one
leg's child."""
import hashlib
import json
import os
import subprocess
import sys

import stream_model as sm
from conftest import ROOT
from dict_streams import check, compare, expected, first_difference  # noqa: F401  (the one oracle comparison, and the one cache)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vector_store as store  # noqa: E402,F401  (how a family lies on disk: the loaders read through it)


def in_batches(pkg, datas, caps, dicts=None, flags=0, what="", size=240, entries=None, where=None):
    """`check` in batches of at most `size` streams -> the results"""
    results = []
    for at in range(0, len(datas), size):
        cut = slice(at, at + size)
        results += check(pkg, datas[cut], caps[cut], dicts and dicts[cut], flags, "%s %d.." % (what, at), entries=entries and entries[cut], where=where)
    return results


# ------------------------------------------------------------------ copies of a stream
def variants(rnd, c, n, recipe="words"):
    """copies of a valid stream of n bytes of output -> (datas, caps).  "words" (test_gpu_engine._variants): exact, one short, half,
    random, roomy; four copies that are truncated or have one or two bits flipped.  "tails": the five buffers of "words" -- its four damaged
    copies are drawn and dropped --, then two truncated copies and two with one bit flipped.  "dict": exact, one short, half, roomy; two
    truncated copies, two with one or two bits flipped."""
    def flipped(d):
        for _ in range(rnd.choice([1, 1, 2])):
            d[rnd.randrange(0, len(d))] ^= 1 << rnd.randrange(8)
        return d
    if recipe == "dict":
        datas, caps = [c] * 4, [n, max(0, n - 1), n // 2, n + 1000]
        for k in range(4):
            d = bytearray(c)
            datas.append(bytes(d[:rnd.randrange(1, max(2, len(d)))] if k < 2 else flipped(d))); caps.append(n + 4096)
        return datas, caps
    datas, caps = [c] * 5, [max(0, cap) for cap in (n, n - 1, n // 2, rnd.randrange(1, max(2, n)), n + 1000)]
    for _ in range(4):
        d = bytearray(c)
        datas.append(bytes(d[:rnd.randrange(1, len(d))] if rnd.random() < 0.4 else flipped(d))); caps.append(n + 4096)
    if recipe == "words":
        return datas, caps
    assert recipe == "tails", recipe
    datas, caps = datas[:5], caps[:5]
    for k in range(2):
        datas.append(c[:rnd.randrange(1, len(c))]); caps.append(n + 4096)
    for k in range(2):
        f = bytearray(c); f[rnd.randrange(len(f))] ^= 1 << rnd.randrange(8)
        datas.append(bytes(f)); caps.append(n + 4096)
    return datas, caps


def take(by, rnd, out, flags_of=lambda e: 0, random_cap=False, named_tag=False):
    """the constructor of a leg set -> take(label, cap=None, damage=None), which appends one stream of `by` (label -> (entry, stream) or
    (entry, stream, dictionary)) to `out`.  damage: "cut" somewhere in the second half, or "flip" one bit in the last two thirds.  cap:
    bytes, or "short", "half", "roomy", and under random_cap "random" -- drawn at every call, asked for or not, which is what keeps
    word_vectors.leg_set the set it was; None: the output's size, with 64 bytes to spare for an invalid or damaged stream.  A changed
    stream's label gets /capacity/damage: the capacity in bytes, under named_tag by the name it was asked for."""
    def one(label, cap=None, damage=None):
        e, c, *d = by[label]
        n = e["size"]
        if damage == "cut":
            c = c[:rnd.randrange(len(c) // 2, len(c))]
        elif damage == "flip":
            x = bytearray(c); x[rnd.randrange(len(x) // 3, len(x))] ^= 1 << rnd.randrange(8); c = bytes(x)
        caps = {None: n if e["valid"] and not damage else n + 64, "short": n - 1, "half": n // 2, "roomy": n + 1000}
        if random_cap:
            caps["random"] = rnd.randrange(1, max(2, n))
        size = caps.get(cap, cap)
        if named_tag:
            tag = "/%s/%s" % (cap, damage) if cap or damage else ""
        else:
            tag = "" if size == n and not damage else "/%s/%s" % (size, damage)
        out.append((label + tag, c, size, flags_of(e), d[0] if d else None))
    return one


# ------------------------------------------------------------------ the legs
LEGS = (("general", {"BROTLI_AMD_GANG": "0"}), ("default", {}), ("gang8", {"BROTLI_AMD_GANG": "8"}), ("scan", {"BROTLI_AMD_ENGINE": "scan"}),
        ("records", {"BROTLI_AMD_NO_SCAN": "1"}), ("checked", {"BROTLI_AMD_NO_SCAN": "1", "BROTLI_AMD_ENGINE": "norecall"}),
        ("norec", {"BROTLI_AMD_NO_SCAN": "1", "BROTLI_AMD_ENGINE": "norec"}))
# a row of a leg: label, result, error_code, decoded_size, consumed, num_commands, num_metablocks, engine_commands, SHA-256, first differing byte
COMMANDS, ENGINE = 5, 7


def child_env(env):
    e = dict(os.environ)
    for k in ("BROTLI_AMD_GANG", "BROTLI_AMD_ENGINE", "BROTLI_AMD_NO_SCAN", "BROTLI_AMD_POOL"):
        e.pop(k, None)
    e.update(env)
    return e


def _leg_child(module, which):
    """decodes MODULE.leg_set() in its two parts (each a batch of its own, which gets gangs of blocks), or MODULE.wide_set() in one, a
    batch per setting of the flags, with no torch in the process -> one line of JSON: the rows, and last_gang() of every batch of flags 0"""
    import importlib
    import importlib.util
    name = "rust_brotli_decompressor_amd"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); sys.modules[name] = pkg; spec.loader.exec_module(pkg)
    m = importlib.import_module(module)
    streams = getattr(m, which)()
    rows, gangs = [], []
    for part in ([streams] if which == "wide_set" else [streams[:m.SPLIT], streams[m.SPLIT:]]):
        for flags in sorted({s[3] for s in part}):
            sel = [s for s in part if s[3] == flags]
            b = pkg.Batch(len(sel))
            res, outs = b.decode_host([s[1] for s in sel], [s[2] for s in sel], flags, dicts=[s[4] for s in sel] if any(s[4] for s in sel) else None)
            if flags == 0:
                gangs.append(b.last_gang())
            b.close()
            for (label, c, cap, _, d), r, o in zip(sel, res, outs):
                rows.append([label, r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands, r.num_metablocks, r.engine_commands,
                             hashlib.sha256(o).hexdigest(), first_difference(o, expected(c, cap, flags, d)[1])])
    print(json.dumps({"rows": rows, "gangs": gangs}))


def run_legs(module, which="leg_set", legs=LEGS, show=lambda label, row: "/" not in label, where=None):
    """MODULE's set in a fresh process per leg, the legs side by side -> {leg: {"rows": {label: row}, "gangs"}}.  Asserted for every leg
    before it returns: a row per stream, the oracle's status words and SHA-256, and the other legs' rows in everything but
    `engine_commands`, which says which path ran (csrc/brotli_device_abi.h) and is printed for the streams that `show` picks.
    where(label, byte) -> what a differing byte belongs to."""
    streams = getattr(module, which)()
    want = {}   # (the oracle is built and its answers are known before the legs, which ask it for the first differing byte, start)
    for label, comp, cap, flags, d in streams:
        info, exp = expected(comp, cap, flags, d)
        want[label] = info, hashlib.sha256(exp).hexdigest()
    assert len(want) == len(streams)
    running = [(name, subprocess.Popen([sys.executable, os.path.abspath(__file__), module.__name__, which], env=child_env(env), stdin=subprocess.DEVNULL,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for name, env in legs]
    got = {}
    try:
        for name, p in running:
            out, err = p.communicate(timeout=600)
            assert p.returncode == 0, (name, err[-2000:])
            got[name] = json.loads(out.strip().splitlines()[-1])
    finally:
        for _, p in running:
            if p.poll() is None:
                p.kill(); p.wait()
    for name, g in got.items():
        print("engine_commands of num_commands,", name, {r[0]: (r[ENGINE], r[COMMANDS]) for r in g["rows"] if show(r[0], r)}, "gangs:", g["gangs"])
    strip = lambda rs: [r[:ENGINE] + r[ENGINE + 1:] for r in rs]   # (everything but engine_commands)
    for name, g in got.items():
        bad = []
        assert len(g["rows"]) == len(streams), (name, len(g["rows"]))
        for r in g["rows"]:
            info, sha = want[r[0]]
            ok = r[1:4] == [info.result, info.error_code, info.decoded_size] and r[8] == sha
            if ok and info.result == 1:
                ok = r[4:7] == [info.consumed, info.num_commands, info.num_metablocks]
            if not ok:
                bad.append((r[:7], (info.result, info.error_code, info.decoded_size, info.consumed, info.num_commands), r[9], where and where(r[0], r[9])))
        assert not bad, (name, len(bad), bad[:8])
        assert strip(g["rows"]) == strip(got[legs[0][0]]["rows"]), name
    return {name: {"rows": {r[0]: r for r in g["rows"]}, "gangs": g["gangs"]} for name, g in got.items()}


def in_a_child(module, function, env):
    """MODULE.FUNCTION(pkg) in a fresh process under child_env(env) -> (what it returned, by way of JSON; the child's stderr)"""
    script = "import sys, json; sys.path.insert(0, sys.argv[1]); import conftest, %s as t; print(json.dumps(t.%s(conftest.load_pkg())))" % (module, function)
    out = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "tests")], env=child_env(env), capture_output=True, text=True, timeout=600,
                         stdin=subprocess.DEVNULL)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


# ------------------------------------------------------------------ recurring test bodies
def limit_caps(size, n):
    """out_cap at every byte from 3 in front of the final copy of n bytes to 1 behind it; for a copy of more than 64 bytes every
    16-byte boundary of the output inside the copy, and the bytes on both sides of it"""
    start = size - n
    caps = set(range(start - 3, start + 1)) | set(range(size - 3, size + 2))
    if n <= 64:
        caps |= set(range(start, size))
    else:
        for p in range((start + 16) // 16 * 16, size, 16):
            caps |= {p - 1, p, p + 1}
    return sorted(caps)


def product_seq(pkg, data, ic, oc, dictionary=None):
    """the stream through a DecoderState, ic bytes of input and oc of room a call -> ([(result, consumed, produced)], the bytes)"""
    st = pkg.DecoderState(large_window=True, dictionary=dictionary)
    outs = []

    def step(pending, cap):
        r = st.decompress_stream(pending, cap)
        outs.append(r[2])
        return r[0], r[1], len(r[2])
    seq = sm.run_schedule(step, data, ic, oc, drain=True)
    st.close()
    return seq, b"".join(outs)


def streamed_like_the_model(pkg, comp, ic, oc, label):
    """through BrotliDecoderDecompressStream: call for call what the model of the reference's driver returns (tests/stream_model.py) -> the bytes"""
    got, out = product_seq(pkg, comp, ic, oc)
    m = sm.ReferenceStream(comp)
    want = sm.run_schedule(lambda pending, cap: m.call(len(pending), cap), comp, ic, oc, drain=True)
    assert got == want, (label, (ic, oc), next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w))
    return out


def stream_set_like_solo(pkg, jobs, names, want):
    """the states of `jobs` stepped by a StreamSet and the same states stepped alone give the same calls and bytes, every one ends in
    success, and the bytes are want[i]"""
    from test_gpu_stream_set import Run
    run, twin = Run(pkg, jobs).run(), Run(pkg, jobs).run(how=lambda k: "solo")
    try:
        for i, n in enumerate(names):
            assert run.seq[i] == twin.seq[i] and run.seq[i][-1][0] == 1, n
            assert run.bytes_of(i) == twin.bytes_of(i) == want[i], n
    finally:
        run.close(); twin.close()


def blocks_a_cu(pkg, vectors, per_cu=4, what="one-wave blocks", where=None, cap_of=lambda e: e["size"]):
    """per_cu * CUs + 1 streams cycling over `vectors` ((entry, stream) or (entry, stream, dictionary)) in one batch, each with room for
    its output; more than four blocks a CU are blocks of one wave whatever the streams are -> (the results, stream i being
    vectors[i % len(vectors)]; how many streams)"""
    import torch
    n = per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 1
    sel = [vectors[i % len(vectors)] for i in range(n)]
    dicts = [v[2] for v in sel] if len(vectors[0]) > 2 else None
    return check(pkg, [v[1] for v in sel], [cap_of(v[0]) for v in sel], dicts, 0, what, entries=[v[0] for v in sel], where=where), n


if __name__ == "__main__":
    _leg_child(*sys.argv[1:3])
