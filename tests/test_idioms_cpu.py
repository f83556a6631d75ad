"""The host side of the operator idioms (csrc/lgs_idioms.h) has no HIP in it: tests/cpp/idioms_main.cpp includes that header alone, is
compiled here with the host C++ compiler and run.  Its cases: the two bound searches on tables of 0, 1, 2 and 7 elements with
duplicates, the record search with leading, middle and trailing empty records at strides 1, 4 and 6, the ordered keys of floats and
ints and their inverses, Layout's 256-byte steps, and every operator layout on three argument sets against the closed formula its
*_workspace_bytes returned before the layouts existed (regions disjoint, aligned, in order)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "languagegroundedsemseg_amd", "csrc")
CASES = ["lower_bound and upper_bound", "last_not_above with empty records", "ordered keys", "Layout::take rounds to 256",
         "operator layouts keep their totals and order"]


def test_idioms_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "idioms")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "idioms_main.cpp"),
                         "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    assert run.stdout.splitlines() == CASES + ["idioms ok: 5 cases"], run.stdout


def test_idioms_header_has_no_hip_include_outside_hipcc():
    """Every #include of a HIP header sits inside an `#if defined(__HIPCC__)` block; what a host compiler sees is system headers and the
    engine's plain C header."""
    depth, hipcc_at, seen, hip_inside = 0, None, [], 0
    for ln in open(os.path.join(CSRC, "lgs_idioms.h")):
        s = ln.strip()
        if re.match(r"#\s*if", s):
            depth += 1
            if hipcc_at is None and "__HIPCC__" in s and "!" not in s:
                hipcc_at = depth
        elif re.match(r"#\s*(else|elif)", s):
            if hipcc_at == depth:
                hipcc_at = None                      # the other branch is what the host compiler reads
        elif re.match(r"#\s*endif", s):
            if hipcc_at == depth:
                hipcc_at = None
            depth -= 1
        elif s.startswith("#include"):
            if hipcc_at is None:
                seen.append(s.split()[1])
            else:
                hip_inside += 1
    assert depth == 0
    assert hip_inside >= 1                            # the section exists: the device part does include the runtime
    assert seen and all("hip" not in i and (i.startswith("<") or i == '"../../include/lgs_engine.h"') for i in seen), seen
    engine = [ln.split()[1] for ln in open(os.path.join(ROOT, "include", "lgs_engine.h")) if ln.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in engine), engine
