"""The data page bodies of DELTA_LENGTH_BYTE_ARRAY columns that pyarrow wrote (tests/golden/dlba_pages/, tools/make_dlba_pages.py) against the
reference (dlba_ref.py) and the host hook: every page decodes to its column -- offsets and bytes --, its lengths are as many as its rows and none
is negative, and their sum is exactly the bytes behind them.  Where pyarrow imports, the pages are written again and compared with the fixtures."""
import importlib.util
import os

import pytest

import dlba_pages
import dlba_ref as ref
from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_dlba_pages", os.path.join(ROOT, "tools", "make_dlba_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _values(offsets, data):
    o = [int.from_bytes(offsets[i:i + 4], "little") for i in range(0, len(offsets), 4)]
    return [data[a:b] for a, b in zip(o, o[1:])]


def test_the_fixtures_hold_what_the_issue_names():
    pages = dlba_pages.load()
    assert {(e["type"], e["version"], e["values"]) for e, _, _, _ in pages} == {(t, v, n) for t in ("string", "binary") for v in (1, 2) for n in (1, 9, 1000, 5000)}
    assert len(pages) == 17   # (and the binary case of long values)
    strings = [x for e, _, o, d in pages if e["type"] == "string" for x in _values(o, d)]
    assert b"" in strings and any(len(x.decode()) < len(x) for x in strings)   # the empty string, and multi-byte UTF-8
    assert max(len(x) for e, _, o, d in pages if e["type"] == "binary" for x in _values(o, d)) == 3000
    for e, body, offsets, data in pages:
        assert len(offsets) == 4 * (e["values"] + 1) and max(len(body), len(offsets), len(data)) <= 40000, e["label"]


def test_the_reference_decodes_the_pages():
    for e, body, offsets, data in dlba_pages.load():
        for column in (ref.column, ref.column_serial):
            got_o, got_d, res = column(body, e["values"])
            assert (res[0], res[2], res[4], res[7:]) == (e["values"], e["values"], ref.OK, (ref.DATA_OK, 0, ref.NONE, len(data), len(data))), e["label"]
            assert res[1] == len(body) - len(data) and ref.offsets_bytes(got_o, 0) == offsets and got_d == data, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = dlba_pages.load()
    src = b"".join(body for _, body, _, _ in pages)
    segs, s_at, o_at, d_at = [], 0, 3, 5
    for e, body, offsets, data in pages:
        segs.append((s_at, len(body), o_at, d_at, len(data), e["values"], 0, 0))
        s_at += len(body)
        o_at += len(offsets) + 1; d_at += len(data) + 1
    got_o, got_d, res = pkg.undlba_host(src, segs, o_at, d_at, src_skew=3, offsets_skew=9, data_skew=7, item_deltas=96, order_seed=5)
    for (e, body, offsets, data), s, r in zip(pages, segs, res):
        assert r == ref.column(body, e["values"])[2] and r[8] == 0 and r[10] == r[11] == len(data), e["label"]
        assert got_o[s[2]:s[2] + len(offsets)] == offsets and got_d[s[3]:s[3] + len(data)] == data, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (body, offsets, data) for e, body, offsets, data in dlba_pages.load()}
    for label, typ, version, values in gen.cases():
        body, offsets, data = fixtures[label]
        assert gen.page(typ, version, values) == body, label
        assert gen.column_arrays(values) == (offsets, data), label
