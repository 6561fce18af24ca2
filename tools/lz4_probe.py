#!/usr/bin/env python3
"""LZ4_RAW against SNAPPY, GZIP and ZSTD on the same column: writes the C3-GZIP
column (int64 timestamps, DELTA_BINARY_PACKED, V2 pages, each delta held for 16
rows so that every page compresses) with pyarrow four ways -- lz4, snappy, gzip,
zstd level 1 -- decodes each (the lz4 file twice: by step A and, as lz4-b, by step B) with the timed stage events of the runtime and
prints, per file, the decompression stage (k_lz4, the snappy kernels,
k_inflate_s + k_inflate, k_zstd) and the whole step in ms and decoded GB/s.

  python tools/lz4_probe.py [--rows N] [--steps K] [--page-size BYTES] [--only lz4,gzip] [--model]

--page-size 1048576 --max-rows-per-page 100000000 is the second shape: pages of
1 MiB (pyarrow's default size; its default of 20 000 rows a page is what cuts
the first shape's pages at 17.5 KiB), few pages for one wave each.  With
--model the host model (tools/lz4_model, built into a temporary directory) also
reports, over a sample of the LZ4 pages, the sequences per page and where the
decoded bytes come from: literals against match bytes.  The library under test
is the one PQG_LIB names, or the tree's."""
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
    # C3's deltas (1000 +- 50), each held for 16 rows (tools/zstd_probe.py: random deltas bit-pack to noise)
    deltas = 1000 + np.repeat(rng.integers(-50, 51, size=(rows + 15) // 16, dtype=np.int64), 16)[:rows]
    deltas[0] = 0
    return np.int64(1_600_000_000_000_000) + np.cumsum(deltas)


def write(vals, compression, page_size, level=None, max_rows=20000):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"ts": pa.array(vals)}), buf, compression=compression, compression_level=level,
                   use_dictionary=False, column_encoding={"ts": "DELTA_BINARY_PACKED"}, data_page_version="2.0",
                   data_page_size=page_size, max_rows_per_page=max_rows, row_group_size=len(vals),
                   write_statistics=False)
    return buf.getvalue()


def page_mix(data, sample=16):
    """(pages sampled, sequences, literal bytes, match bytes, compressed bytes) of LZ4 pages, from the host model"""
    d = tempfile.mkdtemp(prefix="lz4_probe_")
    exe = os.path.join(d, "lz4_model")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                    os.path.join(ROOT, "tools", "lz4_model.cpp"), "-o", exe], check=True)
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
    step = max(len(pages) // sample, 1)
    took = pages[::step][:sample]
    seqs = lit = mat = comp = 0
    for p in took:
        lv = p.def_len + p.rep_len if p.page_type == 3 else 0
        lo = p.payload_offset + lv
        body = chunk[lo:lo + p.compressed_size - lv]
        src = os.path.join(d, "page.lz4")
        open(src, "wb").write(body)
        tok = subprocess.run([exe, "-u", str(p.uncompressed_size - lv), src], capture_output=True, text=True,
                             check=True).stdout.split()
        kv = dict(t.split("=") for t in tok[6:])
        assert tok[1] == "0", tok[:6]
        seqs += int(kv["seqs"])
        lit += int(kv["lit_bytes"])
        mat += int(kv["match_bytes"])
        comp += len(body)
    return len(took), seqs, lit, mat, comp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--page-size", type=int, default=18 * 1024)
    ap.add_argument("--max-rows-per-page", type=int, default=20000)
    ap.add_argument("--only", default="lz4,lz4-b,snappy,gzip,zstd-1")
    ap.add_argument("--model", action="store_true")
    args = ap.parse_args()
    vals = column(args.rows)
    # lz4: k_lz4 (step A); lz4-b: the same file by k_lz4_batch (step B), a context of its own
    kinds = {"lz4": ("lz4", None), "lz4-b": ("lz4", None), "snappy": ("snappy", None), "gzip": ("gzip", None),
             "zstd-1": ("zstd", 1)}
    files = [(k, write(vals, kinds[k][0], args.page_size, kinds[k][1], args.max_rows_per_page)) for k in args.only.split(",")]
    os.environ["PQG_LZ4_BATCH"] = "0"
    dec = pqgpu.GpuDecoder(0)
    os.environ["PQG_LZ4_BATCH"] = "1"
    dec_b = pqgpu.GpuDecoder(0)
    del os.environ["PQG_LZ4_BATCH"]
    dec_a = dec
    try:
        dec_a.L.pqg_set_timing(dec_a.ctx, 1)
        dec_b.L.pqg_set_timing(dec_b.ctx, 1)
        for name, data in files:
            dec = dec_b if name == "lz4-b" else dec_a
            pf = pqgpu.ParquetFile(data)
            dev = dec.upload(pf.data)
            job = pqgpu.device_job(pf, 0, 0, dev)
            best = None
            for _ in range(args.steps + 1):  # the first step sizes the arenas
                r = dec.decode_jobs([job])[0]
                assert r.status == 0, r.status
                t = dec.timings()
                if best is None or t[STAGE_DECOMP] < best[STAGE_DECOMP]:
                    best = t
            got = dec.d2h(r.values, r.values_bytes).view(np.int64)
            assert np.array_equal(got, vals), name
            pages = dec.pages(0)
            page_gb = sum(p.uncompressed_size for p in pages) / 1e9  # what the decompression stage writes
            out_gb = vals.nbytes / 1e9
            print("%-7s file %8.1f MB  pages %5d (%6.1f MB)  decompression %8.3f ms %7.2f GB/s of pages  "
                  "step %8.3f ms %7.2f GB/s of values" % (
                      name, len(data) / 1e6, len(pages), page_gb * 1e3, best[STAGE_DECOMP],
                      page_gb / (best[STAGE_DECOMP] * 1e-3), best[STEP], out_gb / (best[STEP] * 1e-3)), flush=True)
            dec.free(dev)
    finally:
        dec_a.close()
        dec_b.close()
    if args.model and files[0][0] == "lz4":
        k, seqs, lit, mat, comp = page_mix(files[0][1])
        print("lz4     model, %d pages: %.0f sequences per page, %.1f compressed bytes per sequence, literals %d bytes, "
              "matches %d bytes (%.1f %% literals)" % (k, seqs / k, comp / max(seqs, 1), lit, mat,
                                                       100.0 * lit / max(lit + mat, 1)))


if __name__ == "__main__":
    main()
