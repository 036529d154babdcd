#!/usr/bin/env python3
"""Writes tests/golden/dba_pages/: the data page bodies of DELTA_BYTE_ARRAY string and binary column chunks as pyarrow writes them, each with
the column it holds, through tools/vector_store.py.  A case is three entries: the DATA PAGE BODY (the prefix lengths and the suffix lengths as
DELTA_BINARY_PACKED streams, then the suffixes' bytes back to back), and the column as Arrow has it: its int32 offsets and its bytes.

The column is required, uncompressed, without statistics, without a dictionary, one data page.  The body is found in the file by what it must
hold: it is the LAST bytes of the chunk that decode, by the reference (tests/dba_ref.py), to exactly the column -- as many prefix and suffix
lengths as rows, no bad element, the suffix lengths' sum the bytes that follow -- and end at the chunk's end.  tests/test_dba_pages_cpu.py
decodes the fixtures with the reference and the host hook and, where pyarrow imports, writes the pages again and compares them with the
fixtures.

    python3 tools/make_dba_pages.py            # needs pyarrow; rewrites tests/golden/dba_pages/"""
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "dba_pages")
SHAPES = (1, 9, 1000, 5000)   # values
LARGEST = 40000   # bytes: no fixture is larger
STEMS = ["https://example.org/α/", "https://example.org/α/日本/", "https://example.org/b/", "/usr/share/doc/"]


def strings(values):
    """the values of a string case, seeded by its shape and SORTED: a thousand and fewer are paths behind a few long stems -- neighbours share
    twenty bytes and more, repeats and multi-byte UTF-8 are among them, and the empty string is the first --; five thousand are short keys,
    so that their column stays a small fixture"""
    rnd = random.Random("dba string %d" % values)
    if values == 1:
        return ["naïve".encode()]
    out = [""]
    while len(out) < values:
        if values <= 1000:
            s = rnd.choice(STEMS) + "".join(rnd.choice("abcé0123") for _ in range(rnd.randrange(0, 7)))
            while len(s.encode()) > 38:
                s = s[:-1]
        else:
            s = "".join(rnd.choice("abcdefgh") for _ in range(rnd.randrange(1, 8)))
        out += [s] * min(values - len(out), rnd.choice((1, 1, 1, 2, 9)))
    return sorted(s.encode() for s in out)


def cases():
    """(label, type, data page version, values)"""
    for typ in ("string", "binary"):
        for version in (1, 2):
            for n in SHAPES:
                vals = strings(n)
                if typ == "binary":   # bytes that are no UTF-8: every byte moved, which keeps the shared prefixes
                    vals = sorted(bytes((b + 0x7b) & 0xFF for b in v) for v in vals)
                yield "%s_v%d_%d" % (typ, version, n), typ, version, vals
    rnd = random.Random("dba unsorted")
    vals = strings(1000)
    rnd.shuffle(vals)
    yield "string_v2_1000_unsorted", "string", 2, vals
    rnd = random.Random("dba long")
    stem = bytes(rnd.getrandbits(8) for _ in range(2900))
    yield "binary_v1_9_long", "binary", 1, [stem + bytes(rnd.getrandbits(8) for _ in range(100)) for _ in range(9)]


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
    import dba_ref as ref
    import dbp_ref
    pa_type = pa.string() if typ == "string" else pa.binary()
    array = pa.array([v.decode() for v in values] if typ == "string" else values, type=pa_type)
    table = pa.table([array], schema=pa.schema([pa.field("c", pa_type, nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=False, column_encoding={"c": "DELTA_BYTE_ARRAY"}, compression="NONE", write_statistics=False,
                   data_page_version="%d.0" % version, data_page_size=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and not col.has_dictionary_page and "DELTA_BYTE_ARRAY" in col.encodings, (col.compression, col.encodings)
    chunk = raw[col.data_page_offset:col.data_page_offset + col.total_compressed_size]
    want = b"".join(values)
    want_offsets = [0]
    for v in values:
        want_offsets.append(want_offsets[-1] + len(v))
    for s in range(len(chunk) - 10, -1, -1):   # the last bytes that decode to the column and end at the chunk's end
        body = chunk[s:]
        if body[0] != 0x80:   # (a block of 128 values and more: its varint's first byte)
            continue
        walked = dbp_ref.decode(body, 8, 0)[1]
        if walked[4] != ref.OK or walked[0] != len(values):
            continue
        offsets, data, res = ref.column(body, len(values))
        if (res[4], res[12], res[0], res[8], res[2], res[10]) == (ref.OK, ref.OK) + (len(values),) * 4 and res[7] == ref.DATA_OK and res[18] == res[19] and offsets == want_offsets and \
                data == want:
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
