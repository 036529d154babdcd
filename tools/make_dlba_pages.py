#!/usr/bin/env python3
"""Writes tests/golden/dlba_pages/: the data page bodies of DELTA_LENGTH_BYTE_ARRAY string and binary column chunks as pyarrow writes them, each
with the column it holds, through tools/vector_store.py.  A case is three entries: the DATA PAGE BODY (the lengths as a DELTA_BINARY_PACKED
stream, then the values' bytes back to back), and the column as Arrow has it: its int32 offsets and its bytes.

The column is required, uncompressed, without statistics, without a dictionary, one data page.  The body is found in the file by what it must
hold: it is the LAST bytes of the chunk that decode, by the reference (tests/dlba_ref.py), to exactly the column -- as many lengths as rows,
none negative, their sum the bytes that follow -- and end at the chunk's end.  tests/test_dlba_pages_cpu.py decodes the fixtures with the
reference and the host hook and, where pyarrow imports, writes the pages again and compares them with the fixtures.

    python3 tools/make_dlba_pages.py            # needs pyarrow; rewrites tests/golden/dlba_pages/"""
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "dlba_pages")
SHAPES = (1, 9, 1000, 5000)   # values
WORDS = ["", "a", "é", "日本", "naïve", "Ω", "parquet", "a longer string of forty bytes, exactly.."]
LARGEST = 40000   # bytes: no fixture is larger


def strings(values):
    """the values of a string case, seeded by its shape: strings of 0 .. 40 bytes -- the empty string and some multi-byte UTF-8 among them;
    five thousand are short, so that their page stays a small fixture"""
    rnd = random.Random("dlba string %d" % values)
    longest = 40 if values <= 1000 else 5
    out = [w for w in WORDS if len(w.encode()) <= longest][:values]
    if values == 1:
        out = ["naïve"]
    while len(out) < values:
        s = "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz0123456789 _-éßΩ日") for _ in range(rnd.randrange(0, 24 if longest == 40 else 5)))
        while len(s.encode()) > longest:
            s = s[:-1]
        out += [s] * min(values - len(out), rnd.choice((1, 1, 1, 2, 9)))
    rnd.shuffle(out)
    return [s.encode() for s in out]


def cases():
    """(label, type, data page version, values)"""
    for typ in ("string", "binary"):
        for version in (1, 2):
            for n in SHAPES:
                vals = strings(n)
                if typ == "binary":   # bytes that are no UTF-8
                    rnd = random.Random("dlba binary %d" % n)
                    vals = [bytes(rnd.getrandbits(8) for _ in range(len(v))) for v in vals]
                yield "%s_v%d_%d" % (typ, version, n), typ, version, vals
    rnd = random.Random("dlba long")
    long_one, short = bytes(rnd.getrandbits(8) for _ in range(3000)), b"\x00\xff\x80"
    yield "binary_v1_9_long", "binary", 1, [short, long_one, short, short, b"", long_one, short, short, long_one]


def column_arrays(values):
    """-> (the int32 offsets' little-endian bytes, the bytes)"""
    offsets, at = [0], 0
    for v in values:
        at += len(v)
        offsets.append(at)
    return b"".join(o.to_bytes(4, "little") for o in offsets), b"".join(values)


def page(typ, version, values):
    """the data page body of the one column chunk that pyarrow writes for the column"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import dlba_ref as ref
    pa_type = pa.string() if typ == "string" else pa.binary()
    array = pa.array([v.decode() for v in values] if typ == "string" else values, type=pa_type)
    table = pa.table([array], schema=pa.schema([pa.field("c", pa_type, nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=False, column_encoding={"c": "DELTA_LENGTH_BYTE_ARRAY"}, compression="NONE", write_statistics=False,
                   data_page_version="%d.0" % version, data_page_size=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and not col.has_dictionary_page and "DELTA_LENGTH_BYTE_ARRAY" in col.encodings, (col.compression, col.encodings)
    chunk = raw[col.data_page_offset:col.data_page_offset + col.total_compressed_size]
    want = b"".join(values)
    want_offsets = [0]
    for v in values:
        want_offsets.append(want_offsets[-1] + len(v))
    for s in range(len(chunk) - len(want) - 5, -1, -1):   # the last bytes that decode to the column and end at the chunk's end
        body = chunk[s:]
        if body[0] != 0x80:   # (a block of 128 values and more: its varint's first byte)
            continue
        offsets, data, res = ref.column(body, len(values))
        if res[4] == ref.OK and res[0] == res[2] == len(values) and res[8] == 0 and res[10] == res[11] == len(want) and offsets == want_offsets and data == want:
            return body
    raise AssertionError("no data page body that decodes to the column")


def main():
    items = []
    for label, typ, version, values in cases():
        body = page(typ, version, values)
        offsets, data = column_arrays(values)
        items.append(({"label": label, "kind": "page", "type": typ, "version": version, "values": len(values), "csize": len(body)}, body))
        items.append(({"label": label + ".offsets", "kind": "offsets", "csize": len(offsets)}, offsets))
        items.append(({"label": label + ".data", "kind": "data", "csize": len(data)}, data))
    assert max(len(s) for _, s in items) <= LARGEST, max(len(s) for _, s in items)
    vector_store.write(GOLDEN, items)
    print("%d cases, %d bytes" % (len(items) // 3, sum(len(s) for _, s in items)))


if __name__ == "__main__":
    main()
