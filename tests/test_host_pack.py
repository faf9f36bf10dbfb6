"""The pure host layout helpers of the C ABI's unit entry points (csrc/tmpc_host_pack.h: pack_dxul, the
banded lambda gather and the two band-layout conversions) in a stand-alone program (host_pack_check.cpp, its
own main) built with the host compiler's address and undefined-behaviour sanitizers.  No GPU, nothing loaded
into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_host_pack_helpers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "host_pack_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "trajoptmpcreference_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_pack_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "host pack ok" in r.stdout
