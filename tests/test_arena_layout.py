"""The arena layout helper of the device plan (cov-tiles_amd/csrc/covt_arena.h), on the CPU."""
import os
import subprocess

from conftest import ROOT


def test_layout_helper_under_sanitizers(tmp_path):
    """covt_arena.h is plain C++ (g++ compiles it without HIP): 200k random arena declarations in a stand-alone
    program built with AddressSanitizer and UndefinedBehaviorSanitizer -- every member on a 256-byte boundary, in
    declaration order, disjoint, an absent member taking no bytes, bytes() the last end -- and binding an absent
    member aborts."""
    exe = str(tmp_path / "arena_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "arena_layout", "arena_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])
