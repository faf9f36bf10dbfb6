"""The launchers' table from runtime (model id, joint count, chain, precision, QP mode and flags) to template
arguments (csrc/tmpc_dispatch.h: for_nj, for_each_nj, for_model, with_real, with_bool, with_qp_mode) in a stand-alone program
(host_dispatch_check.cpp, its own main, three fake compiled models) built with the host compiler's address and
undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_host_dispatch_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "host_dispatch_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "trajoptmpcreference_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_dispatch_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "host dispatch ok" in r.stdout
