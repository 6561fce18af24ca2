#!/usr/bin/env python3
"""Page checksums on and off on the same file, in one run: pyarrow writes an int32 column with
write_page_checksum=True -- uncompressed PLAIN and snappy with pages of 20 000 rows, and
uncompressed with pages of 1 MiB -- and each file is decoded with verification off and on,
interleaved, with the timed stage events of the runtime.  Per file and setting: the whole step, the
decompression stage (which holds the checksum kernels), the values stage (k_values<0>'s PLAIN copy:
the yardstick that reads the same bytes) and, with verification on, the checksum kernels' own time
(pqg_last_crc_ms: k_crc_plan + k_page_crc + k_crc_fin) in ms and in GB/s of page bytes read.  Each
is the best of --steps steps after a sizing step; --rounds rounds.  pqg_crc32 over one large buffer
gives the tile kernel on its own (plus three launches and a copy-back).

  python tools/crc_probe.py [--rows N] [--steps K] [--rounds R] [--only plain,snappy,big]

The library under test is the one PQG_LIB names, or the tree's."""
import argparse
import io
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402

# pqg_last_timings: the whole step, then scan, list, decompression, setup, walk, levels, nn_scan, values, strings, finalize
STEP, STAGE_DECOMP, STAGE_VALUES = 0, 3, 8
SHAPES = {"plain": ("none", 20000), "snappy": ("snappy", 20000), "big": ("none", 100_000_000)}


def write(vals, codec, max_rows):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"v": pa.array(vals)}), buf, compression=codec, use_dictionary=False,
                   data_page_size=1 << 20, max_rows_per_page=max_rows, row_group_size=len(vals),
                   write_statistics=False, write_page_checksum=True)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", default="plain,snappy,big")
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    # runs of 8 out of 4096 values: snappy shortens them, and no page is all one value
    vals = np.repeat(rng.integers(-2 ** 31, 2 ** 31, 4096).astype(np.int32)[rng.integers(0, 4096, args.rows // 8 + 1)], 8)[:args.rows]
    dec = pqgpu.GpuDecoder(0)
    try:
        dec.L.pqg_set_timing(dec.ctx, 1)
        for shape in args.only.split(","):
            codec, max_rows = SHAPES[shape]
            data = write(vals, codec, max_rows)
            pf = pqgpu.ParquetFile(data)
            dev = dec.upload(pf.data)
            job = pqgpu.device_job(pf, 0, 0, dev)
            for rnd in range(args.rounds):
                for on in (False, True):
                    dec.set_verify_crc(on)
                    best, crc_ms = None, None
                    for _ in range(args.steps + 1):  # the first step sizes the arenas
                        r = dec.decode_jobs([job])[0]
                        assert r.status == 0, r.status
                        t = dec.timings()
                        if best is None or t[STEP] < best[STEP]:
                            best = t
                        if on:
                            ms = dec.last_crc_ms()
                            crc_ms = ms if crc_ms is None else min(crc_ms, ms)
                    pages = dec.pages(0)
                    nbytes = sum(p.compressed_size for p in pages)
                    if rnd == 0:
                        assert dec.d2h(r.values, r.values_bytes).tobytes() == vals.tobytes(), shape
                        crcs = dec.page_crcs(0)
                        assert {c.state for c in crcs} == {1 if on else 3}, shape
                    line = "%-6s crc %-3s round %d  file %7.1f MB  pages %5d  page bytes %7.1f MB  step %8.3f ms  " \
                           "decompression %7.3f ms  values stage %7.3f ms %7.1f GB/s read" % (
                               shape, "on" if on else "off", rnd, len(data) / 1e6, len(pages), nbytes / 1e6, best[STEP],
                               best[STAGE_DECOMP], best[STAGE_VALUES], 4.0 * len(vals) / 1e9 / (best[STAGE_VALUES] * 1e-3))
                    if on:
                        line += "  crc kernels %7.3f ms %7.1f GB/s" % (crc_ms, nbytes / 1e9 / (crc_ms * 1e-3))
                    print(line, flush=True)
            dec.set_verify_crc(False)
            # the kernel alone over the file's bytes: pqg_crc32 (three launches, one copy-back, one sync)
            n = len(data)
            want = zlib.crc32(data)
            best = None
            for _ in range(args.steps + 1):
                t0 = time.perf_counter()
                got = dec.crc32(dev, n)
                dt = time.perf_counter() - t0
                assert got == want
                best = dt if best is None else min(best, dt)
            print("%-6s pqg_crc32 of the file, %7.1f MB: %7.3f ms wall, %7.1f GB/s" % (shape, n / 1e6, best * 1e3, n / 1e9 / best),
                  flush=True)
            dec.free(dev)
    finally:
        dec.close()


if __name__ == "__main__":
    main()
