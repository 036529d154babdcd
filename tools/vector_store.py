"""How the families of hand-emitted streams lie under tests/golden/: a manifest.json of entries, and each entry's stream by its size --
less than 256 bytes in the manifest itself ("hex") or end to end in small.N.bin ("at"), up to MAX_FILE bytes a file ("file"), a longer
one a file per part ("files").  The generators (tools/make_*_vectors.py) write through `write`, the loaders (tests/*_vectors.py) read
through `load`; what an entry says about its stream is the generator's."""
import json
import os

MAX_FILE = 64466  # (the largest file under tests/golden/emitter/; a longer stream is written in parts)
MAX_PARTS = 4


def manifest(directory):
    """manifest.json as it stands: a list of entries, or an object whose "streams" are the entries"""
    return json.load(open(os.path.join(directory, "manifest.json")))


def _read(directory, name):
    return open(os.path.join(directory, name), "rb").read()


def read(directory, e, pack=None):
    """the stream of a manifest entry (pack: small.N.bin end to end, for a caller that reads many)"""
    if "hex" in e:
        comp = bytes.fromhex(e["hex"])
    elif "at" in e:
        pack = _pack(directory) if pack is None else pack
        comp = pack[e["at"]:e["at"] + e["csize"]]
    else:
        comp = b"".join(_read(directory, name) for name in e.get("files", [e.get("file")]))
    assert len(comp) == e["csize"], e["label"]
    return comp


def _pack(directory):
    names = sorted((n for n in os.listdir(directory) if n.startswith("small.")), key=lambda n: int(n.split(".")[1]))
    return b"".join(_read(directory, n) for n in names)


def load(directory):
    """[(manifest entry, stream)] in the manifest's order"""
    entries = manifest(directory)
    if isinstance(entries, dict):
        entries = entries["streams"]
    pack = _pack(directory) if any("at" in e for e in entries) else b""
    return [(e, read(directory, e, pack)) for e in entries]


def write(directory, items, small="hex", style="indent", dictionaries=None):
    """clears the directory, places the stream of each (entry, stream) by its size -- the placement becomes the entry's last key; an
    entry that names its "file" already keeps it -- and writes the manifest.  small: where a stream of less than 256 bytes goes, "hex"
    or "pack".  style: "indent" (an indented list) or "lines" (an entry a line); with `dictionaries` (rows of their own) the manifest
    is an object of "dictionaries" and "streams", a line each.  An entry is complete when the next item is asked for."""
    os.makedirs(directory, exist_ok=True)
    for f in os.listdir(directory):
        os.remove(os.path.join(directory, f))

    def put(name, data):
        open(os.path.join(directory, name), "wb").write(data)
    entries, pack = [], bytearray()
    for e, comp in items:
        if "file" in e:
            put(e["file"], comp)
        elif len(comp) < 256 and small == "hex":
            e["hex"] = comp.hex()
        elif len(comp) < 256:
            e["at"] = len(pack)
            pack += comp
        elif len(comp) <= MAX_FILE:
            e["file"] = "%s.br" % e["label"]
            put(e["file"], comp)
        else:
            e["files"] = ["%s.%d.br" % (e["label"], k) for k in range((len(comp) + MAX_FILE - 1) // MAX_FILE)]
            assert len(e["files"]) <= MAX_PARTS, e["label"]
            for k, name in enumerate(e["files"]):
                put(name, comp[k * MAX_FILE:(k + 1) * MAX_FILE])
        entries.append(e)
    for k in range(0, len(pack), MAX_FILE):
        put("small.%d.bin" % (k // MAX_FILE), pack[k:k + MAX_FILE])
    with open(os.path.join(directory, "manifest.json"), "w") as f:
        if dictionaries is not None:
            f.write('{"dictionaries": [\n' + ",\n".join(json.dumps(d) for d in dictionaries) + '\n], "streams": [\n' + ",\n".join(json.dumps(e) for e in entries) + "\n]}\n")
        elif style == "lines":
            f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries) + "\n]\n")
        else:
            json.dump(entries, f, indent=1)
    return entries
