"""BYTE_STREAM_SPLIT without a GPU: the numpy model the GPU tests judge by (bss_util.encode / decode)
against an independent writer, and k_bss's tile code (pqg_bss.h) run on the host by
tools/bss_model.cpp, which checks every load and store of it against the bytes a part may touch.

The first test passes with or without k_bss: it pins the yardstick (the model, and that the streams'
stride is the page's non-null count), not the decoder."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bss_util as B
import pqtest_util as U
from pqgpu import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

KINDS = {"float32": (abi.FLOAT, 4), "float64": (abi.DOUBLE, 8), "int32": (abi.INT32, 4), "int64": (abi.INT64, 8),
         "float16": (abi.FIXED_LEN_BYTE_ARRAY, 2)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_model_decodes_pyarrow_page(kind):
    """The one BSS page of a pyarrow-written chunk (optional, every 5th value null), found through the
    oracle's page table (which it fills although it answers UNSUPPORTED for the encoding)."""
    import pqgpu
    import parity as P
    n = 1000
    arr = B.arrow_array(kind, n, distinct=1000)
    data = B.write(pa.table({"c": arr}), True, data_page_size=1 << 20)
    pf = pqgpu.ParquetFile(data)
    m = pf.chunk_meta(0, 0)
    ptype, w = KINDS[kind]
    assert m.type == ptype and m.codec == 0
    exp = P.oracle_chunk(pf, 0, 0)
    assert exp.status == abi.STATUS_CODES["UNSUPPORTED"]
    data_pages = [p for p in exp.pages if p.page_type == abi.PAGE_DATA]
    assert len(data_pages) == 1 and data_pages[0].encoding == B.ENC
    p = data_pages[0]
    chunk = bytes(pf.data[m.start:m.start + m.total_compressed_size])
    body = chunk[p.payload_offset:p.payload_offset + p.compressed_size]
    assert p.num_values == n
    dlen = int.from_bytes(body[:4], "little")  # V1, max_def 1: the def levels, then the value bytes
    val = body[4 + dlen:]
    nn = n - arr.null_count
    assert nn == 800 and len(val) == nn * w  # the stride is the non-null count, not num_values
    want = np.asarray(arr.drop_null().to_numpy(zero_copy_only=False)).tobytes()
    assert B.decode(val, nn, w) == want
    assert B.encode(want, w) == val


def test_model_round_trip_widths():
    for w in (1, 2, 3, 4, 8, 12, 16, 17):
        for nn in (0, 1, 17, 255):
            v = B.random_values(nn, w, 1)
            e = B.encode(v, w)
            assert B.decode(e, nn, w) == v
            assert all(e[k * nn + i] == v[i * w + k] for i in range(nn) for k in range(w))


def test_host_model_of_the_kernel(tmp_path):
    """tools/bss_model.cpp: pqg_bss.h's tile code over a sweep of widths, sizes, parts and alignments."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bss_model")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bss_model.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
