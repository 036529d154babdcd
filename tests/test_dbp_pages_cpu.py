"""The page bodies that pyarrow wrote (tests/golden/dbp/, tools/make_dbp_pages.py) against the reference (dbp_ref.py) and the host hook: every
page decodes to its column and ends exactly at the page's end.  Where pyarrow imports, the pages are written again and compared with the
fixtures."""
import importlib.util
import os

import pytest

import dbp_pages
import dbp_ref as ref
from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_dbp_pages", os.path.join(ROOT, "tools", "make_dbp_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixtures_hold_what_the_issue_names():
    pages = dbp_pages.load()
    assert {(e["bits"], e["version"], e["values"]) for e, _, _ in pages} >= {(b, v, n) for b in (32, 64) for v in (1, 2) for n in (1, 2, 70, 131, 257, 258, 1000)}
    assert all(len(column) == e["values"] * e["bits"] // 8 for e, _, column in pages)
    widest = {e["bits"]: max(max(body[o + ref.read_varint(body, o)[1]:][:4]) for o in ref.block_offsets(body)) for e, body, _ in pages if "random" in e["label"]}
    assert widest[64] == 64 and widest[32] >= 32   # the widths reach the type's (INT32 deltas are taken in 32 bits, or wider)
    # a last block with omitted miniblocks
    assert any((e["values"] - 1) % ref.decode(body)[1][5] <= ref.decode(body)[1][5] // 4 and e["values"] > 1 for e, body, _ in pages)


def test_the_reference_decodes_the_pages():
    for e, body, column in dbp_pages.load():
        w = e["bits"] // 8
        for decode in (ref.decode, ref.decode_serial):
            vals, res = decode(body, w)
            assert res[:3] == (e["values"], len(body), e["values"]) and res[4] == ref.OK and res[6] == 4, e["label"]
            assert b"".join(int(v).to_bytes(w, "little") for v in vals) == column, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = dbp_pages.load()
    src = b"".join(body for _, body, _ in pages)
    segs, s_at, d_at = [], 0, 3
    for e, body, column in pages:
        segs.append((s_at, len(body), d_at, e["values"], e["bits"] // 8))
        s_at += len(body)
        d_at += len(column) + 1
    dst, res = pkg.undbp_host(src, segs, d_at, src_skew=3, dst_skew=9, item_deltas=96, order_seed=5)
    for (e, body, column), s, r in zip(pages, segs, res):
        assert r == ref.decode(body, s[4])[1] and dst[s[2]:s[2] + len(column)] == column, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (body, column) for e, body, column in dbp_pages.load()}
    for label, bits, version, values in gen.cases():
        body, column = fixtures[label]
        assert gen.page_body(bits, version, values) == body, label
        assert b"".join((v & ((1 << bits) - 1)).to_bytes(bits // 8, "little") for v in values) == column, label
