#!/usr/bin/env python3
"""Writes tests/golden/null_pages/: the data page of NULLABLE PLAIN column chunks as pyarrow writes them, v1 and v2, each with the column it holds
as values plus a mask, through tools/vector_store.py.  A case is its BODY -- of a v1 page the 4-byte length, the definition levels and the
PLAIN values of the rows that are there; of a v2 page those values alone --, of a v2 page its LEVELS (which that version keeps outside the
compressed body, without a length), the column's rows as little-endian bytes with 0 where a row is null, and the column's validity bitmap
(bit i & 7 of byte i >> 3).

The column is nullable, not dictionary-encoded, uncompressed, without statistics, one data page.  The bodies are found in the file by what they
must hold: the chunk ends with the PLAIN values of the rows that are there; in v1 the four bytes in front of the levels equal their length; in
v2 the levels are the bytes in front of the values that decode to exactly the rows and end there (tests/null_ref.py).  Every column ends in
eight or more rows of one kind, so that its levels end in an RLE run and hold exactly the rows: a writer pads a last bit-packed group to eight
levels, and tensors.outputs_as_tensors refuses a stream whose levels are not exactly its rows.  tests/test_null_pages_cpu.py decodes the
fixtures with the reference and, where pyarrow imports, writes the pages again and compares them with the fixtures.

    python3 tools/make_null_pages.py            # needs pyarrow; rewrites tests/golden/null_pages/"""
import io
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "null_pages")
SHAPES = ("one_null", "nine_some", "thousand_scattered", "five_thousand_runs", "thousand_none")
TYPES = {"int32": ("<i", 4), "int64": ("<q", 8), "float32": ("<f", 4), "float64": ("<d", 8)}


def column(typ, shape):
    """the rows of a case, seeded by its name: a value, or None for a null"""
    rnd = random.Random("%s %s" % (typ, shape))
    value = lambda: rnd.randrange(-1 << 30, 1 << 30) if typ.startswith("int") else struct.unpack("<f", struct.pack("<f", rnd.uniform(-1e6, 1e6)))[0]
    if shape == "one_null":
        return [None]
    if shape == "nine_some":
        return [value() for _ in range(8)] + [None]
    if shape == "thousand_scattered":   # about 30 % nulls, and twelve rows that are there at the end
        return [None if rnd.random() < 0.3 else value() for _ in range(988)] + [value() for _ in range(12)]
    if shape == "five_thousand_runs":   # long runs of nulls and of values, short scattered stretches between them
        out = []
        while len(out) < 5000:
            kind = rnd.random()
            n = rnd.choice((30, 100, 400, 17, 1024))
            out += [None] * n if kind < 0.4 else [value() for _ in range(n)] if kind < 0.8 else [None if rnd.random() < 0.5 else value() for _ in range(rnd.randrange(1, 40))]
        return out[:4980] + [None] * 20
    assert shape == "thousand_none"
    return [value() for _ in range(1000)]


def column_bytes(typ, values):
    """the rows as little-endian bytes, 0 where a row is null"""
    fmt, _ = TYPES[typ]
    return b"".join(struct.pack(fmt, 0 if v is None else v) for v in values)


def mask_bytes(values):
    out = bytearray((len(values) + 7) // 8)
    for i, v in enumerate(values):
        if v is not None:
            out[i >> 3] |= 1 << (i & 7)
    return bytes(out)


def cases():
    """(label, type, data page version, rows)"""
    for typ in TYPES:
        for version in (1, 2):
            for shape in SHAPES:
                yield "%s_v%d_%s" % (typ, version, shape), typ, version, column(typ, shape)


def pages(typ, version, values):
    """(the body, the levels -- b"" for v1, whose body holds them --) of the one data page that pyarrow writes for the column"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import null_ref as ref
    pa_type = {"int32": pa.int32(), "int64": pa.int64(), "float32": pa.float32(), "float64": pa.float64()}[typ]
    table = pa.table([pa.array(values, type=pa_type)], schema=pa.schema([pa.field("c", pa_type, nullable=True)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=False, compression="NONE", write_statistics=False, data_page_version="%d.0" % version, data_page_size=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and not col.has_dictionary_page and "PLAIN" in col.encodings, (col.compression, col.encodings)
    fmt, w = TYPES[typ]
    plain = b"".join(struct.pack(fmt, v) for v in values if v is not None)
    chunk = raw[col.data_page_offset:col.data_page_offset + col.total_compressed_size]
    assert chunk.endswith(plain), "the chunk does not end with the PLAIN values of the rows that are there"
    end = len(chunk) - len(plain)   # where the levels end
    want, want_mask = column_bytes(typ, values), mask_bytes(values)
    present = len(plain) // w
    for s in range(end - 1, -1, -1):   # the levels nearest to the values that decode to exactly the rows and end there
        if version == 1:
            if s < 4 or int.from_bytes(chunk[s - 4:s], "little") != end - s:
                continue
            body, levels = chunk[s - 4:], b""
            slots, valid, res = ref.outputs(body, 1, 1, w, ref.LENGTH_PREFIX | ref.VALUES_FOLLOW, cap=len(values))
        else:
            body, levels = plain, chunk[s:end]
            slots, valid, res = ref.outputs(levels, 1, 1, w, 0, plain, present, cap=len(values))
        if res[3] == ref.OK and res[0] == len(values) and res[5:] == (present, 0, present) and slots == want and valid == want_mask:
            return body, levels
    raise AssertionError("no levels in front of the values that decode to the rows")


def main():
    items = []
    for label, typ, version, values in cases():
        body, levels = pages(typ, version, values)
        w = TYPES[typ][1]
        items.append(({"label": label, "kind": "page", "type": typ, "width": w, "version": version, "rows": len(values), "present": sum(v is not None for v in values),
                       "csize": len(body)}, body))
        if version == 2:
            items.append(({"label": label + ".levels", "kind": "levels", "csize": len(levels)}, levels))
        raw = column_bytes(typ, values)
        items.append(({"label": label + ".column", "kind": "column", "csize": len(raw)}, raw))
        mask = mask_bytes(values)
        items.append(({"label": label + ".mask", "kind": "mask", "csize": len(mask)}, mask))
    vector_store.write(GOLDEN, items)
    print("%d cases, %d bytes" % (sum(1 for e, _ in items if e["kind"] == "page"), sum(len(s) for _, s in items)))


if __name__ == "__main__":
    main()
