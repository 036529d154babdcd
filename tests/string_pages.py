"""tests/golden/string_pages/ (tools/make_string_pages.py): the dictionary page body and the data page body of dictionary-encoded string column
chunks as pyarrow wrote them, each with the column they hold as Arrow has it.  Shared by test_string_pages_cpu.py and test_gpu_undict_bytes.py."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vector_store as store  # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "string_pages")


def load():
    """[(the data page's manifest entry, the dictionary page body, the data page body, the column's int32 offsets as bytes, the column's bytes)]
    in the manifest's order"""
    items = store.load(DIR)
    by_label = {e["label"]: data for e, data in items}
    return [(e, by_label[e["label"] + ".dictionary"], data, by_label[e["label"] + ".offsets"], by_label[e["label"] + ".data"]) for e, data in items if e["kind"] == "page"]
