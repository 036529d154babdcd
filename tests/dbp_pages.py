"""tests/golden/dbp/ (tools/make_dbp_pages.py): DELTA_BINARY_PACKED page bodies as pyarrow wrote them, each with the column it holds.
Shared by test_dbp_pages_cpu.py and test_gpu_undbp.py."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vector_store as store  # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "dbp")


def load():
    """[(the page's manifest entry, the page body, the column's little-endian bytes)] in the manifest's order"""
    items = store.load(DIR)
    columns = {e["label"]: data for e, data in items if e["kind"] == "column"}
    return [(e, data, columns[e["label"] + ".column"]) for e, data in items if e["kind"] == "page"]
