"""K9s without a GPU: the lane code of pqg_filter / pqg_select (pqg_filter.h) run on the host by
tools/filter_model.cpp, 64 lanes one after another, against a plain scalar loop, with every load
and store checked against the inputs and outputs.  Built and run as a stand-alone program, plain
and under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_host_model_of_the_kernels(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "filter_model")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-I",
                    os.path.join(ROOT, "parquet-go_amd", "csrc"), os.path.join(ROOT, "tools", "filter_model.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
