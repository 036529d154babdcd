#!/usr/bin/env python3
"""Writes tests/golden/string_pages/: the two pages of dictionary-encoded (RLE_DICTIONARY) STRING column chunks as pyarrow writes them, each with
the column it holds, through tools/vector_store.py.  A case is four entries: the DICTIONARY PAGE BODY (the distinct values as PLAIN byte arrays:
a 4-byte length, then the bytes), the DATA PAGE BODY (a width byte k, then the RLE / bit-packed hybrid of k-bit indices), and the column as
Arrow has it: its int32 offsets and its bytes.

The column is required, uncompressed, without statistics, one data page.  The bodies are found in the file by what they must hold: the
dictionary page body is the distinct values in the order of their first appearance, PLAIN, somewhere in the chunk; the data page body is the
LAST bytes of the chunk that begin with the width byte and decode, through that dictionary, to exactly the column (tests/dict_bytes_ref.py),
ending at the chunk's end.  tests/test_string_pages_cpu.py decodes the fixtures with the reference and the host hook and, where pyarrow
imports, writes the pages again and compares them with the fixtures.

    python3 tools/make_string_pages.py            # needs pyarrow; rewrites tests/golden/string_pages/"""
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "string_pages")
SHAPES = ((1, 1), (9, 2), (1000, 200), (5000, 5000))   # (values, distinct)
WORDS = ["", "a", "é", "日本", "naïve", "Ω", "parquet", "a longer string of forty bytes, exactly.."]
LARGEST = 40000   # bytes: no fixture is larger than the largest one of tests/golden/dict_pages/


def strings(values, distinct):
    """the values of a string case, seeded by its shape: `distinct` different ones of 0 .. 40 bytes -- the empty string and some multi-byte
    UTF-8 among them; five thousand distinct ones are short, so that their dictionary page stays a small fixture --, each at least once,
    repeats in runs and scattered"""
    rnd = random.Random("string %d %d" % (values, distinct))
    longest = 40 if distinct < 1000 else 5
    pool, seen = [], set()
    for w in WORDS:
        if len(pool) < distinct and len(w.encode()) <= longest:
            pool.append(w); seen.add(w)
    while len(pool) < distinct:
        s = "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz0123456789 _-éßΩ日") for _ in range(rnd.randrange(1, 24 if longest == 40 else 5)))
        while len(s.encode()) > longest:
            s = s[:-1]
        if s not in seen:
            pool.append(s); seen.add(s)
    rnd.shuffle(pool)
    out = list(pool)
    while len(out) < values:
        out += [rnd.choice(pool)] * min(values - len(out), rnd.choice((1, 1, 1, 2, 9, 40)))
    if distinct < values:
        head = out[:distinct]; rest = out[distinct:]
        out = head[:1] + rest[:len(rest) // 2] + head[1:] + rest[len(rest) // 2:]
    return [s.encode() for s in out]


def cases():
    """(label, type, data page version, values)"""
    for version in (1, 2):
        for n, d in SHAPES:
            yield "string_v%d_%d_%d" % (version, n, d), "string", version, strings(n, d)
    rnd = random.Random("binary")
    long_one, short = bytes(rnd.getrandbits(8) for _ in range(3000)), b"\x00\xff\x80"
    yield "binary_v1_9_2", "binary", 1, [short, long_one, short, short, short, long_one, short, short, long_one]


def column_arrays(values):
    """-> (the int32 offsets' little-endian bytes, the bytes)"""
    offsets, at = [0], 0
    for v in values:
        at += len(v)
        offsets.append(at)
    return b"".join(o.to_bytes(4, "little") for o in offsets), b"".join(values)


def pages(typ, version, values):
    """(the dictionary page body, the data page body) of the one column chunk that pyarrow writes for the column"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import dict_bytes_ref as ref
    pa_type = pa.string() if typ == "string" else pa.binary()
    array = pa.array([v.decode() for v in values] if typ == "string" else values, type=pa_type)
    table = pa.table([array], schema=pa.schema([pa.field("c", pa_type, nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=True, compression="NONE", write_statistics=False, data_page_version="%d.0" % version,
                   data_page_size=1 << 30, dictionary_pagesize_limit=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and col.has_dictionary_page and "RLE_DICTIONARY" in col.encodings, (col.compression, col.encodings)
    seen, distinct = set(), []
    for v in values:
        if v not in seen:
            seen.add(v); distinct.append(v)
    plain = ref.dictionary_bytes(distinct)
    start = min(col.dictionary_page_offset, col.data_page_offset)
    chunk = raw[start:start + col.total_compressed_size]
    at = chunk.find(plain)
    assert at >= 0, "no PLAIN dictionary of the distinct values in the chunk"
    want = b"".join(values)
    for s in range(len(chunk) - 1, at + len(plain) - 1, -1):   # the last bytes that decode to the column and end at the chunk's end
        body = chunk[s:]
        if body[0] > 32:
            continue
        offsets, data, res = ref.column(body, 0, ref.WIDTH_BYTE, plain, len(distinct), len(values))
        if res[3] == ref.OK and res[1] == len(body) and res[5] == 0 and len(values) <= res[0] < len(values) + 8 and data == want:
            return plain, body
    raise AssertionError("no data page body that decodes to the column")


def main():
    items = []
    for label, typ, version, values in cases():
        plain, body = pages(typ, version, values)
        distinct = len(set(values))
        offsets, data = column_arrays(values)
        items.append(({"label": label + ".dictionary", "kind": "dictionary", "entries": distinct, "csize": len(plain)}, plain))
        items.append(({"label": label, "kind": "page", "type": typ, "version": version, "values": len(values), "distinct": distinct, "bits": body[0], "csize": len(body)}, body))
        items.append(({"label": label + ".offsets", "kind": "offsets", "csize": len(offsets)}, offsets))
        items.append(({"label": label + ".data", "kind": "data", "csize": len(data)}, data))
    assert max(len(s) for _, s in items) <= LARGEST, max(len(s) for _, s in items)
    vector_store.write(GOLDEN, items)
    print("%d cases, %d bytes" % (len(items) // 4, sum(len(s) for _, s in items)))


if __name__ == "__main__":
    main()
