#!/usr/bin/env python3
"""Writes tests/golden/dbp/: DELTA_BINARY_PACKED page bodies as pyarrow writes them, each with the column it holds, through
tools/vector_store.py.  A page entry's stream is the page body; the entry behind it holds the column's little-endian bytes.

The column is required, uncompressed, without dictionary and without statistics, one page; the body is the bytes from the header pattern
`B M N zigzag(first)` (B = 128 or 256, M = 4) to data_page_offset + total_compressed_size.  tests/test_dbp_pages_cpu.py decodes the fixtures with
the reference and, where pyarrow imports, writes the pages again and compares them with the fixtures.

    python3 tools/make_dbp_pages.py            # needs pyarrow; rewrites tests/golden/dbp/"""
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vector_store  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "dbp")
COUNTS = (1, 2, 70, 131, 257, 258, 1000)


def column(bits, n, kind):
    """the values of a case: seeded by its name"""
    rnd = random.Random("%d %d %s" % (bits, n, kind))
    top = 1 << (bits - 1)
    if kind == "random":   # the full range: the widths reach the type's
        return [rnd.randrange(-top, top) for _ in range(n)]
    v, out = rnd.randrange(1 << 20), []   # sorted ids with a jump now and then: small widths, and miniblocks of 0 bits
    for i in range(n):
        out.append(v)
        v += 3 if i % 97 else rnd.randrange(1 << 14)
    return out


def cases():
    """(label, bits, data page version, values)"""
    for bits in (32, 64):
        for version in (1, 2):
            for n in COUNTS:
                yield "int%d_v%d_%d" % (bits, version, n), bits, version, column(bits, n, "ids")
        yield "int%d_v2_1000_random" % bits, bits, 2, column(bits, 1000, "random")


def page_body(bits, version, values):
    """the body of the one data page that pyarrow writes for the column"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import dbp_ref as ref
    typ = pa.int32() if bits == 32 else pa.int64()
    table = pa.table([pa.array(values, type=typ)], schema=pa.schema([pa.field("c", typ, nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(table, buf, use_dictionary=False, compression="NONE", write_statistics=False, column_encoding={"c": "DELTA_BINARY_PACKED"},
                   data_page_version="%d.0" % version, data_page_size=1 << 30)
    raw = buf.getvalue()
    col = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(0).column(0)
    assert col.compression == "UNCOMPRESSED" and not col.has_dictionary_page and "DELTA_BINARY_PACKED" in col.encodings
    page = raw[col.data_page_offset:col.data_page_offset + col.total_compressed_size]
    starts = [page.find(ref.varint(B) + ref.varint(4) + ref.varint(len(values)) + ref.varint(ref.zigzag(values[0]))) for B in (128, 256)]
    starts = [s for s in starts if s >= 0]
    assert starts, "no DELTA_BINARY_PACKED header in the page"
    return page[min(starts):]


def main():
    items = []
    for label, bits, version, values in cases():
        body = page_body(bits, version, values)
        items.append(({"label": label, "kind": "page", "bits": bits, "version": version, "values": len(values), "csize": len(body)}, body))
        raw = b"".join((v & ((1 << bits) - 1)).to_bytes(bits // 8, "little") for v in values)
        items.append(({"label": label + ".column", "kind": "column", "bits": bits, "csize": len(raw)}, raw))
    vector_store.write(GOLDEN, items)
    print("%d pages, %d bytes" % (len(items) // 2, sum(len(s) for _, s in items)))


if __name__ == "__main__":
    main()
