"""The dictionary and data page bodies that pyarrow wrote (tests/golden/dict_pages/, tools/make_dict_pages.py) against the reference (dict_ref.py)
and the host hook: every data page, through its dictionary page, decodes to its column and ends exactly at the page's end, with no index outside
the dictionary.  Where pyarrow imports, the pages are written again and compared with the fixtures."""
import importlib.util
import os

import pytest

import dict_pages
import dict_ref as ref
from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_dict_pages", os.path.join(ROOT, "tools", "make_dict_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixtures_hold_what_the_issue_names():
    pages = dict_pages.load()
    assert len(pages) == 32
    assert {(e["type"], e["version"], e["values"], e["distinct"]) for e, _, _, _ in pages} == {
        (t, v, n, d) for t in ("int32", "int64", "float32", "float64") for v in (1, 2) for n, d in ((1, 1), (9, 2), (1000, 200), (5000, 5000))}
    # (this writer gives a dictionary of ONE entry fields of 1 bit, not of 0: k = 0 is the hand-made vectors' to cover)
    assert {(e["distinct"], e["bits"]) for e, _, _, _ in pages} == {(1, 1), (2, 1), (200, 8), (5000, 13)}
    assert all(len(column) == e["values"] * e["width"] and len(dictionary) == e["distinct"] * e["width"] and body[0] == e["bits"]
               for e, dictionary, body, column in pages)
    assert max(len(x) for p in pages for x in p[1:]) <= 64 << 10   # (small, as the fixtures around them are)


def test_the_reference_decodes_the_pages():
    for e, dictionary, body, column in dict_pages.load():
        vals, res = ref.decode(body, 0, e["width"], ref.WIDTH_BYTE, dictionary, e["distinct"])
        assert res[1:] == (len(body), res[2], ref.OK, e["bits"], 0, ref.NONE) and e["values"] <= res[0] < e["values"] + 8, e["label"]
        assert vals[:e["values"]].astype("<u%d" % e["width"]).tobytes() == column, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = dict_pages.load()
    src = b"".join(body for _, _, body, _ in pages)
    table = b"".join(dictionary for _, dictionary, _, _ in pages)
    segs, s_at, d_at, t_at = [], 0, 3, 0
    for e, dictionary, body, column in pages:
        segs.append((s_at, len(body), d_at, e["values"], 99, e["width"], ref.WIDTH_BYTE, t_at, e["distinct"]))
        s_at += len(body); t_at += len(dictionary)
        d_at += len(column) + 1
    dst, res = pkg.undict_host(src, table, segs, d_at, src_skew=3, dst_skew=9, dict_skew=5, item_elems=96, order_seed=5)
    for (e, dictionary, body, column), s, r in zip(pages, segs, res):
        assert r == ref.decode(body, 0, e["width"], ref.WIDTH_BYTE, dictionary, e["distinct"], e["values"])[1] and r[5] == 0, e["label"]
        assert dst[s[2]:s[2] + len(column)] == column, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (dictionary, body, column) for e, dictionary, body, column in dict_pages.load()}
    for label, typ, version, values, distinct in gen.cases():
        dictionary, body, column = fixtures[label]
        assert gen.pages(typ, version, values) == (dictionary, body), label
        assert gen.column_bytes(typ, values) == column, label
