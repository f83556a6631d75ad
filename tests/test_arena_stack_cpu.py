"""The arena's bump stack (csrc/lgs_arena.h) is host arithmetic with no HIP in it: tests/cpp/arena_stack_main.cpp includes that header
alone, is compiled here with the host C++ compiler and run.  Its cases: a full block refuses cleanly, release in allocation order
pops at the last release, reverse order pops each time, a hole under a live block, unknown offsets, the peak, the 256-byte rounding."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "languagegroundedsemseg_amd", "csrc")
CASES = ["full block fails cleanly", "allocation order pops at the last release", "reverse order pops each time", "hole under a live block",
         "unknown offset is ignored", "peak is the high-water mark", "sizes round up to 256"]


def test_arena_stack_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "arena_stack")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "arena_stack_main.cpp"),
                         "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    assert run.stdout.splitlines() == CASES + ["arena stack ok: 7 cases"], run.stdout


def test_arena_header_has_no_hip_include():
    includes = [ln.split()[1] for ln in open(os.path.join(CSRC, "lgs_arena.h")) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes   # system headers only
