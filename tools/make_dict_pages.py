#!/usr/bin/env python3
"""Writes tests/golden/dict_pages/: the two pages of dictionary-encoded (RLE_DICTIONARY) column chunks as pyarrow writes them, each with the column
it holds, through tools/vector_store.py.  A case is three entries: the DICTIONARY PAGE BODY (the distinct values, PLAIN), the DATA PAGE BODY (a
width byte k, then the RLE / bit-packed hybrid of k-bit indices) and the column's little-endian bytes.

The column is required, uncompressed, without statistics, one data page.  The bodies are found in the file by what they must hold: the
dictionary page body is the distinct values in the order of their first appearance, PLAIN, somewhere between the chunk's dictionary_page_offset
and data_page_offset; the data page body is the LAST bytes of the chunk that begin with the width byte and decode, through that dictionary, to
exactly the column (tests/dict_ref.py), ending at the chunk's end.  tests/test_dict_pages_cpu.py decodes the fixtures with the reference and,
where pyarrow imports, writes the pages again and compares them with the fixtures.

    python3 tools/make_dict_pages.py            # needs pyarrow; rewrites tests/golden/dict_pages/"""
import io
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "dict_pages")
SHAPES = ((1, 1), (9, 2), (1000, 200), (5000, 5000))   # (values, distinct): k = 0, 1, 8, 13
TYPES = {"int32": ("<i", 4), "int64": ("<q", 8), "float32": ("<f", 4), "float64": ("<d", 8)}


def column(typ, values, distinct):
    """the values of a case, seeded by its name: `distinct` different ones, each at least once, repeats in runs and scattered"""
    rnd = random.Random("%s %d %d" % (typ, values, distinct))
    pool = set()
    while len(pool) < distinct:
        pool.add(rnd.randrange(-1 << 30, 1 << 30) if typ.startswith("int") else struct.unpack("<f", struct.pack("<f", rnd.uniform(-1e6, 1e6)))[0])
    pool = sorted(pool)
    rnd.shuffle(pool)
    out = list(pool)
    while len(out) < values:
        out += [rnd.choice(pool)] * min(values - len(out), rnd.choice((1, 1, 1, 2, 9, 40)))
    if distinct < values:
        head = out[:distinct]; rest = out[distinct:]
        out = head[:1] + rest[:len(rest) // 2] + head[1:] + rest[len(rest) // 2:]
    return out


def column_bytes(typ, values):
    fmt, _ = TYPES[typ]
    return b"".join(struct.pack(fmt, v) for v in values)


def cases():
    """(label, type, data page version, values, distinct)"""
    for typ in TYPES:
        for version in (1, 2):
            for n, d in SHAPES:
                yield "%s_v%d_%d_%d" % (typ, version, n, d), typ, version, column(typ, n, d), d


def pages(typ, version, values):
    """(the dictionary page body, the data page body) of the one column chunk that pyarrow writes for the column"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import dict_ref as ref
    pa_type = {"int32": pa.int32(), "int64": pa.int64(), "float32": pa.float32(), "float64": pa.float64()}[typ]
    table = pa.table([pa.array(values, type=pa_type)], schema=pa.schema([pa.field("c", pa_type, nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=True, compression="NONE", write_statistics=False, data_page_version="%d.0" % version,
                   data_page_size=1 << 30, dictionary_pagesize_limit=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and col.has_dictionary_page and "RLE_DICTIONARY" in col.encodings, (col.compression, col.encodings)
    w = TYPES[typ][1]
    seen, distinct = set(), []
    for v in values:
        if v not in seen:
            seen.add(v); distinct.append(v)
    plain = column_bytes(typ, distinct)
    start = min(col.dictionary_page_offset, col.data_page_offset)
    chunk = raw[start:start + col.total_compressed_size]
    at = chunk.find(plain)
    assert at >= 0, "no PLAIN dictionary of the distinct values in the chunk"
    want = column_bytes(typ, values)
    for s in range(len(chunk) - 1, at + len(plain) - 1, -1):   # the last bytes that decode to the column and end at the chunk's end
        body = chunk[s:]
        if body[0] > 32:
            continue
        elems, res = ref.elements_bytes(body, 0, w, ref.WIDTH_BYTE, plain, len(distinct), len(values))
        if res[3] == ref.OK and res[1] == len(body) and res[5] == 0 and len(values) <= res[0] < len(values) + 8 and elems == want:
            return plain, body
    raise AssertionError("no data page body that decodes to the column")


def main():
    items = []
    for label, typ, version, values, distinct in cases():
        plain, body = pages(typ, version, values)
        w = TYPES[typ][1]
        items.append(({"label": label + ".dictionary", "kind": "dictionary", "width": w, "entries": len(plain) // w, "csize": len(plain)}, plain))
        items.append(({"label": label, "kind": "page", "type": typ, "width": w, "version": version, "values": len(values), "distinct": distinct, "bits": body[0],
                       "csize": len(body)}, body))
        raw = column_bytes(typ, values)
        items.append(({"label": label + ".column", "kind": "column", "csize": len(raw)}, raw))
    vector_store.write(GOLDEN, items)
    print("%d cases, %d bytes" % (len(items) // 3, sum(len(s) for _, s in items)))


if __name__ == "__main__":
    main()
