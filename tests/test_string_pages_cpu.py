"""The dictionary and data page bodies of string columns that pyarrow wrote (tests/golden/string_pages/, tools/make_string_pages.py) against the
reference (dict_bytes_ref.py) and the host hook: every data page, through its dictionary page, decodes to its column -- offsets and bytes -- and
ends exactly at the page's end, with no index outside the dictionary and no cut dictionary.  Where pyarrow imports, the pages are written again
and compared with the fixtures."""
import importlib.util
import os

import pytest

import dict_bytes_ref as ref
import string_pages
from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_string_pages", os.path.join(ROOT, "tools", "make_string_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixtures_hold_what_the_issue_names():
    pages = string_pages.load()
    assert {(e["type"], e["version"], e["values"], e["distinct"]) for e, _, _, _, _ in pages} == {
        ("string", v, n, d) for v in (1, 2) for n, d in ((1, 1), (9, 2), (1000, 200), (5000, 5000))} | {("binary", 1, 9, 2)}
    for e, dictionary, body, offsets, data in pages:
        entries, consumed, status = ref.parse_dictionary(dictionary)
        assert (len(entries), consumed, status) == (e["distinct"], len(dictionary), ref.DICT_OK) and body[0] == e["bits"] and len(offsets) == 4 * (e["values"] + 1), e["label"]
        if e["type"] == "string":
            assert all(len(x) <= 40 for x in entries) and all(x.decode() is not None for x in entries), e["label"]
    strings = [x for e, d, _, _, _ in pages if e["type"] == "string" for x in ref.parse_dictionary(d)[0]]
    assert b"" in strings and any(len(x.decode()) < len(x) for x in strings)   # the empty string, and multi-byte UTF-8
    assert max(len(x) for e, d, _, _, _ in pages if e["type"] == "binary" for x in ref.parse_dictionary(d)[0]) == 3000
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", "dict_pages", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden", "dict_pages")))
    assert max(len(x) for p in pages for x in p[1:]) <= largest


def test_the_reference_decodes_the_pages():
    for e, dictionary, body, offsets, data in string_pages.load():
        got_o, got_d, res = ref.column(body, 0, ref.WIDTH_BYTE, dictionary, e["distinct"], e["values"])
        assert res[1:7] == (len(body), res[2], ref.OK, e["bits"], 0, ref.NONE) and e["values"] <= res[0] < e["values"] + 8, e["label"]
        assert res[7:] == (len(data), e["distinct"], len(dictionary), ref.DICT_OK), e["label"]
        assert ref.offsets_bytes(got_o, 0) == offsets and got_d == data, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = string_pages.load()
    src = b"".join(body for _, _, body, _, _ in pages)
    table = b"".join(dictionary for _, dictionary, _, _, _ in pages)
    segs, s_at, o_at, d_at, t_at = [], 0, 3, 5, 0
    for e, dictionary, body, offsets, data in pages:
        segs.append((s_at, len(body), o_at, d_at, len(data), e["values"], 0, t_at, len(dictionary), e["distinct"], 99, ref.WIDTH_BYTE))
        s_at += len(body); t_at += len(dictionary)
        o_at += len(offsets) + 1; d_at += len(data) + 1
    got_o, got_d, res, walks = pkg.undict_bytes_host(src, table, segs, o_at, d_at, src_skew=3, offsets_skew=9, data_skew=7, dict_skew=5, item_elems=96, order_seed=5, word_seed=3)
    assert walks == len(pages)
    for (e, dictionary, body, offsets, data), s, r in zip(pages, segs, res):
        assert r == ref.column(body, 0, ref.WIDTH_BYTE, dictionary, e["distinct"], e["values"])[2] and r[5] == 0 and r[10] == ref.DICT_OK, e["label"]
        assert got_o[s[2]:s[2] + len(offsets)] == offsets and got_d[s[3]:s[3] + len(data)] == data, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (dictionary, body, offsets, data) for e, dictionary, body, offsets, data in string_pages.load()}
    for label, typ, version, values in gen.cases():
        dictionary, body, offsets, data = fixtures[label]
        assert gen.pages(typ, version, values) == (dictionary, body), label
        assert gen.column_arrays(values) == (offsets, data), label
