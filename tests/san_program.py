"""The programs of tests/tools/*_san.cpp: headers of csrc/ under AddressSanitizer and UBSan, each a program of its own with its own main."""
import os
import subprocess

from conftest import ROOT


def run(name, tmp_path, args=()):
    """compiles tests/tools/<name>.cpp into tmp_path and runs it with args; asserts that it exited 0 -> the finished process (stdout, stderr as text)"""
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", name + ".cpp"), "-o", exe])
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r
