"""tests/golden/dba_pages/ (tools/make_dba_pages.py): the data page bodies of DELTA_BYTE_ARRAY string and binary column chunks as pyarrow wrote
them, each with the column it holds as Arrow has it.  Shared by test_dba_pages_cpu.py and test_gpu_undba.py."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vector_store as store  # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "dba_pages")


def load():
    """[(the page's manifest entry, the data page body, the column's int32 offsets as bytes, the column's bytes)] in the manifest's order"""
    items = store.load(DIR)
    by_label = {e["label"]: data for e, data in items}
    return [(e, data, by_label[e["label"] + ".offsets"], by_label[e["label"] + ".data"]) for e, data in items if e["kind"] == "page"]
