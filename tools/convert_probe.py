#!/usr/bin/env python3
"""pqg_convert against the values stage on the same column: pyarrow writes optional decimals (about
10 % nulls, PLAIN, uncompressed) as FIXED_LEN_BYTE_ARRAY of 5, 13 and 16 bytes -- decimal128(11,2),
(30,2) and (38,0) -- and one INT96 timestamp column of the same length.  Each file is decoded with
the timed stage events of the runtime and its dense values are converted.  Per file: the values
stage (k_values<0>'s PLAIN copy) in ms and in GB/s of 2 x nn x w, pqg_convert's device time in ms
and in GB/s of nn x (w + out_width) -- the bytes either pass reads plus the bytes it writes -- and
the host's numpy conversion of the same downloaded bytes.  Best of --steps steps after a sizing
step, all in one run on one GPU.

  python tools/convert_probe.py [--rows N] [--steps K] [--only flba5,flba13,flba16,int96]

The library under test is the one PQG_LIB names, or the tree's."""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402
from pqgpu import abi  # noqa: E402
from pqgpu.logical import conversion  # noqa: E402

STEP, STAGE_VALUES = 0, 8  # pqg_last_timings: the whole step, ..., values
# name -> (precision, scale, bits of the random unscaled values)
DECIMALS = {"flba5": (11, 2, 36), "flba13": (30, 2, 99), "flba16": (38, 0, 126)}


def column(kind, rows, seed=5):
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    mask = rng.random(rows) < 0.1
    validity = pa.array(~mask).buffers()[1]
    if kind == "int96":
        ns = rng.integers(-2 ** 62, 2 ** 62, rows)
        return pa.Array.from_buffers(pa.timestamp("ns"), rows, [validity, pa.py_buffer(ns)], null_count=int(mask.sum()))
    p, s, bits = DECIMALS[kind]
    # 128-bit two's complement from two random words, arithmetically shifted down to `bits` bits
    v = np.empty((rows, 2), np.int64)
    hi = rng.integers(-2 ** 63, 2 ** 63, rows)
    lo = rng.integers(0, 2 ** 64, rows, dtype=np.uint64)
    if bits <= 64:
        v[:, 0] = hi >> (64 - bits)
        v[:, 1] = v[:, 0] >> 63
    else:
        v[:, 0] = lo.view(np.int64)
        v[:, 1] = hi >> (128 - bits)
    return pa.Array.from_buffers(pa.decimal128(p, s), rows, [validity, pa.py_buffer(v)], null_count=int(mask.sum()))


def write(arr, int96):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"v": arr}), buf, compression="NONE", use_dictionary=False, row_group_size=len(arr),
                   write_statistics=False, use_deprecated_int96_timestamps=int96)
    return buf.getvalue()


def host_convert(raw, cv):
    """numpy's version of the conversion, on the downloaded dense values."""
    n = len(raw) // cv.in_width
    v = raw.reshape(n, cv.in_width)
    if cv.kind == abi.CONV_INT96_TIME:
        nanos = np.ascontiguousarray(v[:, :8]).view("<u8").reshape(-1)
        day = np.ascontiguousarray(v[:, 8:]).view("<i4").reshape(-1).astype(np.int64)
        return ((day - 2440588) * 86400000000000 + nanos.view(np.int64)).view(np.uint8)
    out = np.empty((n, cv.out_width), np.uint8)
    out[:, :cv.in_width] = v[:, ::-1]
    out[:, cv.in_width:] = (v[:, :1] >> 7) * 0xff
    return out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="flba5,flba13,flba16,int96")
    args = ap.parse_args()
    dec = pqgpu.GpuDecoder(0)
    try:
        dec.L.pqg_set_timing(dec.ctx, 1)
        for kind in args.only.split(","):
            arr = column(kind, args.rows)
            data = write(arr, kind == "int96")
            pf = pqgpu.ParquetFile(data)
            cv = conversion(pf.columns[0].desc, pf.logical_types[0])
            w, ow = cv.in_width, cv.out_width
            dev = dec.upload(pf.data)
            job = pqgpu.device_job(pf, 0, 0, dev)
            best_v = best_c = None
            out = None
            for _ in range(args.steps + 1):  # the first step sizes the arenas
                r = dec.decode_jobs([job])[0]
                assert r.status == 0 and r.value_width == w, (r.status, r.value_width)
                t = dec.timings()[STAGE_VALUES]
                if out is not None:
                    dec.free(out)
                out = dec.convert(r.values, r.num_values, r.values_bytes, cv.kind, w, ow, cv.unit)
                c = dec.last_convert_ms()
                best_v = t if best_v is None else min(best_v, t)
                best_c = c if best_c is None else min(best_c, c)
            nn = r.num_values
            raw = dec.d2h(r.values, r.values_bytes)
            got = dec.d2h(out, nn * ow)
            t0 = time.perf_counter()
            want = host_convert(raw, cv)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(got, want), kind
            if kind == "int96":
                assert np.array_equal(got.view("<i8"), arr.drop_null().cast("int64").to_numpy())
            else:
                assert got.tobytes() == arr.drop_null().buffers()[1].to_pybytes()[:nn * 16]
            print("%-6s w %2d -> %2d  file %7.1f MB  nn %9d  values stage %7.3f ms %7.1f GB/s  pqg_convert %7.3f ms "
                  "%7.1f GB/s  (%.2f of the values stage's rate)  numpy on the host %8.1f ms" % (
                      kind, w, ow, len(data) / 1e6, nn, best_v, 2.0 * nn * w / 1e6 / best_v, best_c,
                      nn * (w + ow) / 1e6 / best_c, (nn * (w + ow) / best_c) / (2.0 * nn * w / best_v), host_ms),
                  flush=True)
            dec.free(out)
            dec.free(dev)
    finally:
        dec.close()


if __name__ == "__main__":
    main()
