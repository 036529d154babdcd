#!/usr/bin/env python3
"""tests/golden/reference_tables.json: digests of the RFC 7932 tables as the reference's sources hold them
(src/context.rs, src/transform.rs, src/dictionary/mod.rs), for tests/test_tables_vs_reference.py.

usage: python tools/make_reference_tables.py <reference checkout>

Only a length and a SHA-256 per table are written, never the tables: a list of numbers is hashed as its decimal values
joined by commas, the dictionary as its 122784 bytes, and the 121 transforms as "<prefix hex>:<type>:<suffix hex>"
joined by commas, with the names of src/transform.rs resolved to affix strings and numbers.
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_tables.json")


def _ints(text):
    return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", text)]


def _rust_array(src, name):
    m = re.search(r"%s\s*:\s*\[[^=]*=\s*\[(.*?)\];" % re.escape(name), src, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return _ints(re.sub(r"//[^\n]*", "", body))


def _digest(values):
    return {"n": len(values), "sha256": hashlib.sha256(",".join(map(str, values)).encode()).hexdigest()}


def _cstr(pool, off):
    return pool[off:pool.index(b"\0", off)]


def main(ref):
    src_dir = os.path.join(ref, "src")
    context = open(os.path.join(src_dir, "context.rs")).read()
    dictionary = open(os.path.join(src_dir, "dictionary", "mod.rs")).read()
    transform = open(os.path.join(src_dir, "transform.rs")).read()
    consts = {k: int(v) for k, v in re.findall(r"const\s+(k\w+)\s*:\s*u8\s*=\s*(\d+)\s*;", transform)}
    entries = re.findall(r"prefix_id:\s*(\w+),\s*transform:\s*(\w+),\s*suffix_id:\s*(\w+),", transform)
    pool = bytes(_rust_array(transform, "kPrefixSuffix"))
    words = bytes(_rust_array(dictionary, "kBrotliDictionary"))
    out = {
        "source": "src/context.rs, src/transform.rs, src/dictionary/mod.rs of the reference (tools/make_reference_tables.py)",
        "kContextLookup": _digest(_rust_array(context, "kContextLookup")),
        "kBrotliDictionaryOffsetsByLength": _digest(_rust_array(dictionary, "kBrotliDictionaryOffsetsByLength")),
        "kBrotliDictionarySizeBitsByLength": _digest(_rust_array(dictionary, "kBrotliDictionarySizeBitsByLength")),
        "kBrotliDictionary": {"n": len(words), "sha256": hashlib.sha256(words).hexdigest()},
        "transforms": _digest(["%s:%d:%s" % (_cstr(pool, consts[p]).hex(), consts[t], _cstr(pool, consts[s]).hex()) for p, t, s in entries]),
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
