#!/usr/bin/env python3
"""tools/isa_compare.py [-v] <old.s> <new.s>: two gfx950 assembly files (hipcc --save-temps, *-hip-amdgcn-*.s) function by function.

Functions are paired in emission order.  Comments and directives are dropped; local labels are numbered by first appearance
inside their function and symbols by the position of their definition in the file, so renamed functions and shifted label
numbers compare equal.  One row a function: same / DIFF, the two instruction counts, the resource lines where they differ
(all of them on the first file's side otherwise).  -v: a unified diff of the functions that differ.  Exit status 1 on any
difference."""
import difflib
import re
import shutil
import subprocess
import sys

RES = re.compile(r"^; (codeLenInByte|(?:Total)?NumSgprs|NumVgprs|ScratchSize)\b[ =:]+(\d+)")


def functions(path):
    """[(symbol, [instruction and label lines], {resource: value})] in emission order."""
    out, cur = [], None
    for line in open(path):
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            cur = (m.group(1), [], {})
            out.append(cur)
            continue
        if cur is None:
            continue
        r = RES.match(line)
        if r:
            cur[2][r.group(1).replace("Total", "")] = int(r.group(2))
        elif not cur[2] and not line.startswith(".Lfunc_end"):
            code = line.split(";")[0].strip()
            if code and not code.startswith(".") or re.match(r"\.L\w+:", code):
                cur[1].append(code)
    order = {name: i for i, (name, _, _) in enumerate(out)}
    for name, body, _ in out:
        labels = {}
        for i, code in enumerate(body):
            code = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), code)
            body[i] = re.sub(r"\b_Z\w+", lambda m: "@f%d" % order[m.group(0)] if m.group(0) in order else m.group(0), code)
        if body and body[0] == name + ":":
            del body[0]
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool:
        return names
    return subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()


def main(argv):
    verbose = "-v" in argv
    paths = [a for a in argv if a != "-v"]
    if len(paths) != 2:
        sys.exit(__doc__)
    old, new = functions(paths[0]), functions(paths[1])
    names = demangle([f[0] for f in new] + [f[0] for f in old[len(new):]])
    differ = len(old) != len(new)
    if differ:
        print("functions: %d against %d" % (len(old), len(new)))
    for i, name in enumerate(names):
        o = old[i] if i < len(old) else (None, [], {})
        n = new[i] if i < len(new) else (None, [], {})
        count = lambda f: sum(not c.endswith(":") for c in f[1])
        same = o[1] == n[1] and o[2] == n[2] and o[0] is not None and n[0] is not None
        differ |= not same
        res = " ".join("%s %s" % (k, o[2].get(k) if o[2].get(k) == n[2].get(k) else "%s->%s" % (o[2].get(k), n[2].get(k)))
                       for k in ("NumVgprs", "NumSgprs", "ScratchSize", "codeLenInByte"))
        print("%-4s %6d %6d  %s  %s" % ("same" if same else "DIFF", count(o), count(n), res, name.replace("(anonymous namespace)::", "")))
        if verbose and not same:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(o[1], n[1], str(o[0]), str(n[0]), lineterm="", n=3))
    print("total %d %d instructions" % tuple(sum(not c.endswith(":") for f in fs for c in f[1]) for fs in (old, new)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
