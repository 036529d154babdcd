"""The data page bodies of DELTA_BYTE_ARRAY columns that pyarrow wrote (tests/golden/dba_pages/, tools/make_dba_pages.py) against the reference
(dba_ref.py) and the host hook: every page decodes to its column -- offsets and bytes --, its prefix and suffix lengths are as many as its rows,
no element breaks a rule, and the suffix lengths' sum is exactly the bytes behind them.  Where pyarrow imports, the pages are written again and
compared with the fixtures."""
import importlib.util
import os

import pytest

import dba_pages
import dba_ref as ref
import dbp_ref
from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_dba_pages", os.path.join(ROOT, "tools", "make_dba_pages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _values(offsets, data):
    o = [int.from_bytes(offsets[i:i + 4], "little") for i in range(0, len(offsets), 4)]
    return [data[a:b] for a, b in zip(o, o[1:])]


def test_the_fixtures_hold_what_the_issue_names():
    pages = dba_pages.load()
    shapes = {(t, v, n) for t in ("string", "binary") for v in (1, 2) for n in (1, 9, 1000, 5000)}
    assert shapes <= {(e["type"], e["version"], e["values"]) for e, _, _, _ in pages} and len(pages) == 18   # (and the unsorted and the long case)
    by_label = {e["label"]: (body, _values(o, d)) for e, body, o, d in pages}
    # sorted values with long shared prefixes, multi-byte UTF-8 and the empty string among them
    body, values = by_label["string_v1_1000"]
    prefixes = [int(v) for v in dbp_ref.decode(body, 8)[0]]
    assert values == sorted(values) and b"" in values and any(len(x.decode()) < len(x) for x in values) and sorted(prefixes)[len(prefixes) // 2] >= 20
    # an unsorted case
    body, values = by_label["string_v2_1000_unsorted"]
    assert values != sorted(values) and sorted(values) == by_label["string_v2_1000"][1]
    # values of 3000 bytes that share 2900
    body, values = by_label["binary_v1_9_long"]
    assert {len(x) for x in values} == {3000} and min(int(v) for v in dbp_ref.decode(body, 8)[0][1:]) >= 2900
    for e, body, offsets, data in pages:
        assert len(offsets) == 4 * (e["values"] + 1) and max(len(body), len(offsets), len(data)) <= 40000, e["label"]


def test_the_reference_decodes_the_pages():
    for e, body, offsets, data in dba_pages.load():
        got_o, got_d, res = ref.column(body, e["values"])
        n = e["values"]
        assert (res[0], res[2], res[4], res[8], res[10], res[12]) == (n, n, ref.OK, n, n, ref.OK), e["label"]
        assert res[7] == ref.DATA_OK and res[15:] == (ref.BAD_NONE, ref.NONE, len(data), res[19], res[19]), e["label"]
        assert res[1] + res[9] + res[19] == len(body) and ref.offsets_bytes(got_o, 0) == offsets and got_d == data, e["label"]


def test_the_host_hook_decodes_the_pages(pkg):
    pages = dba_pages.load()
    src = b"".join(body for _, body, _, _ in pages)
    segs, s_at, o_at, d_at = [], 0, 3, 5
    for e, body, offsets, data in pages:
        segs.append((s_at, len(body), o_at, d_at, len(data), e["values"], 0, 0))
        s_at += len(body)
        o_at += len(offsets) + 1; d_at += len(data) + 1
    for item, seed in ((96, 5), (0, 0)):
        got_o, got_d, res = pkg.undba_host(src, segs, o_at, d_at, src_skew=3, offsets_skew=9, data_skew=7, item_deltas=item, order_seed=seed)
        for (e, body, offsets, data), s, r in zip(pages, segs, res):
            assert r == ref.column(body, e["values"])[2] and r[ref.R_FIRST_BAD] == ref.NONE and r[ref.R_BYTES] == len(data), e["label"]
            assert got_o[s[2]:s[2] + len(offsets)] == offsets and got_d[s[3]:s[3] + len(data)] == data, e["label"]


def test_pyarrow_writes_the_same_pages():
    pytest.importorskip("pyarrow")
    gen = _generator()
    fixtures = {e["label"]: (body, offsets, data) for e, body, offsets, data in dba_pages.load()}
    for label, typ, version, values in gen.cases():
        body, offsets, data = fixtures[label]
        assert gen.page(typ, version, values) == body, label
        assert gen.column_arrays(values) == (offsets, data), label
