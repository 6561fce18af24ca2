"""The bytewise four-positions-per-dword run-header parse of the 1-bit level
decoder (l1_quad / l1_quad_codes, pqg_lev1_parse.h) against the byte-wise
l1_hdr, on the host: builds tools/lev1_quad_check.cpp and runs it (every
(b0, b1, b2) in every byte lane, neighbouring lanes 0x00 / 0xff / random)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quad_parse_matches_bytewise_parse(tmp_path):
    exe = str(tmp_path / "lev1_quad_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall",
                    "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                    os.path.join(ROOT, "tools", "lev1_quad_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " 0 errors" in r.stdout
