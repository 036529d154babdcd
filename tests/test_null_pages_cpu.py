"""The nullable data pages that pyarrow wrote (tests/golden/null_pages/, tools/make_null_pages.py) against the reference (null_ref.py) and the host
hook: every page's levels and values decode to its column and its validity bitmap, the levels hold exactly the rows, every row that is there has a
value and none is left over.  Where pyarrow imports, the pages are written again and compared with the fixtures."""
import importlib.util
import os

import pytest

import null_pages
import null_ref as ref
from conftest import ROOT

PF = ref.LENGTH_PREFIX | ref.VALUES_FOLLOW


def _generator():
    spec = importlib.util.spec_from_file_location("make_null_pages", os.path.join(ROOT, "tools", "make_null_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _decode(e, body, levels, cap=None):
    if e["version"] == 1:
        return ref.outputs(body, 1, 1, e["width"], PF, cap=cap)
    return ref.outputs(levels, 1, 1, e["width"], 0, body, len(body) // e["width"], cap=cap)


def test_the_fixtures_hold_what_the_issue_names():
    pages = null_pages.load()
    assert len(pages) == 40
    assert {(e["type"], e["version"], e["rows"]) for e, *_ in pages} == {(t, v, n) for t in ("int32", "int64", "float32", "float64") for v in (1, 2) for n in (1, 9, 1000, 5000)}
    by_shape = {(e["rows"], e["present"] == e["rows"], e["present"] == 0) for e, *_ in pages}
    assert by_shape == {(1, False, True), (9, False, False), (1000, False, False), (1000, True, False), (5000, False, False)}
    assert all(0.25 < 1 - e["present"] / e["rows"] < 0.35 for e, *_ in pages if "scattered" in e["label"])
    for e, body, levels, column, mask in pages:
        assert len(column) == e["rows"] * e["width"] and len(mask) == (e["rows"] + 7) // 8, e["label"]
        assert (len(levels) == 0) == (e["version"] == 1), e["label"]
        if e["version"] == 1:
            L = int.from_bytes(body[:4], "little")
            assert len(body) == 4 + L + e["present"] * e["width"], e["label"]
        else:
            assert len(body) == e["present"] * e["width"], e["label"]
    root = os.path.join(ROOT, "tests", "golden", "null_pages")
    assert max(os.path.getsize(os.path.join(root, f)) for f in os.listdir(root)) <= 64 << 10   # (small, as the fixtures around them are)


def test_the_reference_decodes_the_pages():
    for e, body, levels, column, mask in null_pages.load():
        slots, valid, res = _decode(e, body, levels)
        assert res[0] == e["rows"] and res[3] == ref.OK and res[4] == 1 and res[5:] == (e["present"], 0, e["present"]), e["label"]
        assert res[1] == (len(body) - e["present"] * e["width"] if e["version"] == 1 else len(levels)), e["label"]
        assert slots == column and valid == mask, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = null_pages.load()
    src, values, segs, d_at, b_at = bytearray(), bytearray(), [], 3, 1
    for e, body, levels, column, mask in pages:
        if e["version"] == 1:
            segs.append((len(src), len(body), d_at, e["rows"], 1, e["width"], PF, 1, 0, 0, b_at))
            src += body
        else:
            segs.append((len(src), len(levels), d_at, e["rows"], 1, e["width"], 0, 1, len(values), e["present"], b_at))
            src += levels
            values += body
        d_at += len(column) + 1
        b_at += len(mask) + 1
    dst, bits, res = pkg.unnull_host(bytes(src), bytes(values), segs, d_at, b_at, src_skew=3, dst_skew=9, values_skew=5, valid_skew=7, item_elems=96, order_seed=5)
    for (e, body, levels, column, mask), s, r in zip(pages, segs, res):
        assert r == _decode(e, body, levels, e["rows"])[2] and r[5:] == (e["present"], 0, e["present"]), e["label"]
        assert dst[s[2]:s[2] + len(column)] == column and bits[s[10]:s[10] + len(mask)] == mask, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (body, levels, column, mask) for e, body, levels, column, mask in null_pages.load()}
    for label, typ, version, values in gen.cases():
        body, levels, column, mask = fixtures[label]
        assert gen.pages(typ, version, values) == (body, levels), label
        assert gen.column_bytes(typ, values) == column and gen.mask_bytes(values) == mask, label
