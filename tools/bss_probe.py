#!/usr/bin/env python3
"""BYTE_STREAM_SPLIT against PLAIN on the same column: pyarrow writes one column shape twice, PLAIN
and BYTE_STREAM_SPLIT -- float32 and float64, optional with about 10 % nulls, uncompressed and
zstd level 1 -- and each file is decoded with the timed stage events of the runtime.  Per file: the
values stage (k_values<0>'s PLAIN copy, or k_bss) in ms and in GB/s of 2 x nn x w (the bytes either
stage reads plus the bytes it writes), and the whole step.  Each file is measured --rounds times
(best of --steps steps after a sizing step, each time), all in one run on one GPU.

  python tools/bss_probe.py [--rows N] [--steps K] [--rounds R] [--page-size BYTES] [--max-rows-per-page N]
                            [--only float32,float64] [--codecs none,zstd] [--counters]

pyarrow's default of 20 000 rows a page cuts the pages long before 1 MiB: one part per page.
--max-rows-per-page 100000000 gives pages of 1 MiB (262 144 or 131 072 slots), which the values
stage cuts into parts of 4096 values when they hold more than 65 536.

With --counters and a -DPQG_PROFILE library (PQG_LIB=.../libpqgpu_prof.so) the phase counters of
pqg_bss.hip are printed after each BSS file: cycles summed over the waves in part set-up, loads +
stage, transpose and stores, and the tiles and parts they cover.  The library under test is the one
PQG_LIB names, or the tree's."""
import argparse
import ctypes as C
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402

# pqg_last_timings: the whole step, then scan, list, decompression, setup, walk, levels, nn_scan, values, strings, finalize
STEP, STAGE_DECOMP, STAGE_VALUES = 0, 3, 8
BSS_COUNTERS = 192  # pqg_debug_counters: the slots of pqg_bss.hip


def column(kind, rows, seed=5):
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    vals = np.round(rng.standard_normal(rows) * 100, 2).astype(np.float32 if kind == "float32" else np.float64)
    return pa.array(vals, mask=rng.random(rows) < 0.1)


def write(arr, split, codec, page_size, max_rows):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"v": arr}), buf, compression=codec, compression_level=1 if codec == "zstd" else None,
                   use_dictionary=False, use_byte_stream_split=split, data_page_size=page_size,
                   max_rows_per_page=max_rows, row_group_size=len(arr), write_statistics=False)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--page-size", type=int, default=1 << 20)
    ap.add_argument("--max-rows-per-page", type=int, default=20000)
    ap.add_argument("--only", default="float32,float64")
    ap.add_argument("--codecs", default="none,zstd")
    ap.add_argument("--counters", action="store_true")
    args = ap.parse_args()
    dec = pqgpu.GpuDecoder(0)
    try:
        dec.L.pqg_set_timing(dec.ctx, 1)
        for kind in args.only.split(","):
            arr = column(kind, args.rows)
            w = 4 if kind == "float32" else 8
            want = np.asarray(arr.drop_null().to_numpy()).tobytes()
            nn = len(want) // w
            for codec in args.codecs.split(","):
                for enc, split in (("plain", False), ("bss", True)):
                    data = write(arr, split, codec, args.page_size, args.max_rows_per_page)
                    pf = pqgpu.ParquetFile(data)
                    dev = dec.upload(pf.data)
                    job = pqgpu.device_job(pf, 0, 0, dev)
                    for rnd in range(args.rounds):
                        best = None
                        for _ in range(args.steps + 1):  # the first step sizes the arenas
                            r = dec.decode_jobs([job])[0]
                            assert r.status == 0, r.status
                            t = dec.timings()
                            if best is None or t[STAGE_VALUES] < best[STAGE_VALUES]:
                                best = t
                        if rnd == 0:
                            assert dec.d2h(r.values, r.values_bytes).tobytes() == want, (kind, codec, enc)
                            pages = dec.pages(0)
                            assert {p.encoding for p in pages} == {9 if split else 0}
                        print("%-7s %-5s %-5s round %d  file %7.1f MB  pages %5d  nn %9d  values stage %7.3f ms %8.1f GB/s"
                              "  decompression %7.3f ms  step %8.3f ms" % (
                                  kind, codec, enc, rnd, len(data) / 1e6, len(pages), nn, best[STAGE_VALUES],
                                  2.0 * nn * w / 1e9 / (best[STAGE_VALUES] * 1e-3), best[STAGE_DECOMP], best[STEP]),
                              flush=True)
                    if args.counters and split:
                        out = (C.c_uint64 * 224)()
                        k = dec.L.pqg_debug_counters(dec.ctx, out, 224)  # read + reset; 0: not a PQG_PROFILE library
                        if k >= BSS_COUNTERS + 8:
                            c = [out[BSS_COUNTERS + i] for i in range(8)]
                            print("        k_bss cycles over all steps: set-up %d  loads+stage %d  transpose %d  stores %d  "
                                  "tiles %d  parts %d  in parts %d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6]), flush=True)
                    dec.free(dev)
    finally:
        dec.close()


if __name__ == "__main__":
    main()
