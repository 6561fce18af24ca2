#!/usr/bin/env python3
"""ZSTD against GZIP on the same column: writes the C3-GZIP column (int64
timestamps, DELTA_BINARY_PACKED, V2 pages) with pyarrow three ways -- ZSTD
level 1, ZSTD level 3, GZIP -- decodes each with the timed stage events of the
runtime and prints, per file, the decompression stage (k_zstd, or k_inflate_s +
k_inflate) and the whole step in ms and decoded GB/s.

  python tools/zstd_probe.py [--rows N] [--steps K]

With --model the host model (tools/zstd_model, built into a temporary
directory) also reports where the decoded bytes of a sample of pages come from:
literals against match bytes."""
import argparse
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402

# pqg_last_timings: the whole step, then scan, list, decompression, setup, walk, levels, nn_scan, values, strings, finalize
STEP, STAGE_DECOMP = 0, 3


def column(rows, seed=3):
    rng = np.random.default_rng(seed)
    # C3's deltas (1000 +- 50), each held for 16 rows: random deltas bit-pack to noise, which no codec
    # shrinks, and pyarrow then stores the V2 page raw with is_compressed=false (Q4: such a page fails)
    deltas = 1000 + np.repeat(rng.integers(-50, 51, size=(rows + 15) // 16, dtype=np.int64), 16)[:rows]
    deltas[0] = 0
    return np.int64(1_600_000_000_000_000) + np.cumsum(deltas)


def write(vals, compression, level=None):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"ts": pa.array(vals)}), buf, compression=compression, compression_level=level,
                   use_dictionary=False, column_encoding={"ts": "DELTA_BINARY_PACKED"}, data_page_version="2.0",
                   data_page_size=18 * 1024, row_group_size=len(vals), write_statistics=False)
    return buf.getvalue()


def page_mix(data, sample=8):
    """literal and match bytes of the first `sample` ZSTD pages, from the host model"""
    d = tempfile.mkdtemp(prefix="zstd_probe_")
    exe = os.path.join(d, "zstd_model")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                    os.path.join(ROOT, "tools", "zstd_model.cpp"), "-o", exe], check=True)
    pf = pqgpu.ParquetFile(data)
    dec = pqgpu.GpuDecoder(0)
    try:
        dev = dec.upload(pf.data)
        dec.decode_jobs([pqgpu.device_job(pf, 0, 0, dev)])
        pages = dec.pages(0)
    finally:
        dec.close()
    job, _ = pf.host_job(0, 0)
    chunk = C.string_at(job.data, job.data_len)  # payload offsets are relative to the chunk's first byte
    lit = mat = 0
    for p in pages[:sample]:
        lv = p.def_len + p.rep_len if p.page_type == 3 else 0
        lo = p.payload_offset + lv
        body = chunk[lo:lo + p.compressed_size - lv]
        src = os.path.join(d, "page.zst")
        open(src, "wb").write(body)
        tok = subprocess.run([exe, src], capture_output=True, text=True, check=True).stdout.split()
        kv = dict(t.split("=") for t in tok[6:])
        assert tok[1] == "0", tok[:6]
        lit += int(kv["lit_bytes"])
        mat += int(kv["match_bytes"])
    return lit, mat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--model", action="store_true")
    args = ap.parse_args()
    vals = column(args.rows)
    files = [("zstd-1", write(vals, "zstd", 1)), ("zstd-3", write(vals, "zstd", 3)), ("gzip", write(vals, "gzip"))]
    dec = pqgpu.GpuDecoder(0)
    try:
        dec.L.pqg_set_timing(dec.ctx, 1)
        for name, data in files:
            pf = pqgpu.ParquetFile(data)
            dev = dec.upload(pf.data)
            job = pqgpu.device_job(pf, 0, 0, dev)
            best = None
            for _ in range(args.steps + 1):  # the first step sizes the arenas
                r = dec.decode_jobs([job])[0]
                assert r.status == 0, r.status
                t = dec.timings()
                if best is None or t[STEP] < best[STEP]:
                    best = t
            got = dec.d2h(r.values, r.values_bytes).view(np.int64)
            assert np.array_equal(got, vals), name
            out_gb = vals.nbytes / 1e9
            print("%-7s file %8.1f MB  pages %5d  decompression %8.3f ms %7.2f GB/s  step %8.3f ms %7.2f GB/s" % (
                name, len(data) / 1e6, len(dec.pages(0)), best[STAGE_DECOMP], out_gb / (best[STAGE_DECOMP] * 1e-3),
                best[STEP], out_gb / (best[STEP] * 1e-3)), flush=True)
            dec.free(dev)
    finally:
        dec.close()
    if args.model:
        for name, data in files[:2]:
            lit, mat = page_mix(data)
            print("%-7s model, first pages: literals %d bytes, matches %d bytes (%.1f %% literals)" % (
                name, lit, mat, 100.0 * lit / max(lit + mat, 1)))


if __name__ == "__main__":
    main()
