"""tests/golden/null_pages/ (tools/make_null_pages.py): the data page of nullable PLAIN column chunks as pyarrow wrote them, v1 and v2, each with the
column it holds as values plus a mask.  Shared by test_null_pages_cpu.py and test_gpu_unnull.py."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vector_store as store  # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "null_pages")


def load():
    """[(the page's manifest entry, the body, the levels -- b"" for v1, whose body holds them --, the rows' little-endian bytes with 0 at a null,
    the validity bitmap)] in the manifest's order"""
    items = store.load(DIR)
    by_label = {e["label"]: data for e, data in items}
    return [(e, data, by_label.get(e["label"] + ".levels", b""), by_label[e["label"] + ".column"], by_label[e["label"] + ".mask"]) for e, data in items if e["kind"] == "page"]
